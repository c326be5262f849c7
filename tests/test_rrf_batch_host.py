"""pvs_rrf_search_batch on the host side: declared, exported, bound, and the wrapper's argument checks (no device needed)."""
import os
import re
import subprocess

import numpy as np
import pytest

import panoptikon_amd as pvs
from panoptikon_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rrf_search_batch_is_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pvs.h")).read(), flags=re.S)
    assert re.search(r"\bpvs_rrf_search_batch\s*\(", header)
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH], text=True)
    assert re.search(r"\bT pvs_rrf_search_batch\b", out)
    assert "pvs_rrf_search_batch" in L.SYMBOLS
    assert "rrf_search_batch" in pvs.__all__


class _FakeIndex:
    """Stands in for a VectorIndex: the wrapper must reject the call before it reaches the library or a device."""

    def __init__(self, dim):
        self.dim = dim
        self._h = None

    def _queries(self, q):
        raise AssertionError("the wrapper reached the library")


def test_rrf_search_batch_rejects_mismatched_batches_before_the_library():
    a, b = _FakeIndex(8), _FakeIndex(16)
    with pytest.raises(ValueError, match="same number of queries"):
        pvs.rrf_search_batch([dict(index=a, query=np.zeros((3, 8), np.float32), metric=pvs.COSINE),
                              dict(index=b, query=np.zeros((4, 16), np.float32), metric=pvs.L2)], 10)
    with pytest.raises(ValueError, match="dimension"):
        pvs.rrf_search_batch([dict(index=a, query=np.zeros((3, 9), np.float32), metric=pvs.COSINE)], 10)
    with pytest.raises(ValueError, match=r"\[batch, dim\]"):
        pvs.rrf_search_batch([dict(index=a, query=np.zeros(8, np.float32), metric=pvs.COSINE)], 10)
    with pytest.raises(ValueError):
        pvs.rrf_search_batch([], 10)
