#!/usr/bin/env python3
"""What the device does between two consecutive shared (256-query) passes B, from a rocprofv3 rocpd database of the default
bench.py region.  For every pass B followed by another one: the ends of the first and the last pass C kernel behind it, the idle time
from the first one's end to the next query prep, the prep / pass A / k-th select kernels before the next pass B, and the whole gap from one pass B's end to the next
one's start.  Usage: pair_tail_rocpd.py results.db [out.md] [min_pass_b_us (default 1500)]"""
import sqlite3
import statistics
import sys

db = sys.argv[1]
min_b = float(sys.argv[3]) if len(sys.argv) > 3 else 1500.0
c = sqlite3.connect(db)
cols = [r[1] for r in c.execute("pragma table_info(rocpd_kernel_dispatch)")]
qcol = "d.queue_id" if "queue_id" in cols else "0"
rows = [(st / 1e3, en / 1e3, name, q) for st, en, name, q in c.execute(
    f"""select d.start, d.end, s.kernel_name, {qcol} from rocpd_kernel_dispatch d
        join rocpd_info_kernel_symbol s on d.kernel_id = s.id order by d.start""")]


def kind(name, dur):
    if "k_scan_wide" in name or "k_scan" in name:
        return "B" if dur >= min_b else "A"
    for key, k in (("k_finalize", "C"), ("k_prep_queries", "prep"), ("k_kth", "kth")):
        if key in name:
            return k
    return "other"


ev = [(st, en, kind(name, en - st), q) for st, en, name, q in rows]
bs = [i for i, e in enumerate(ev) if e[2] == "B"]
out = ["| pair | B us | B end -> first C end us | B end -> last C end us | C kernels (us) | idle before prep us | prep us | pass A us | k_kth us | prep -> next B start us | B end -> next B start us |",
       "|---|---|---|---|---|---|---|---|---|---|---|"]
agg = {"first_c": [], "tail_c": [], "idle": [], "prelude": [], "gap": [], "b": []}
for n, (i, j) in enumerate(zip(bs, bs[1:])):
    b, nb = ev[i], ev[j]
    between = [e for e in ev[i + 1:j]]
    cs = [e for e in between if e[2] == "C"]
    c_end = max((e[1] for e in cs), default=b[1])
    c_first = min((e[1] for e in cs), default=b[1])
    preps = [e for e in between if e[2] == "prep" and e[0] >= b[1]]
    first_prep = min((e[0] for e in preps), default=nb[0])
    a_us = sum(e[1] - e[0] for e in between if e[2] == "A")
    kth_us = sum(e[1] - e[0] for e in between if e[2] == "kth")
    prep_us = sum(e[1] - e[0] for e in preps)
    tail_c = c_end - b[1]
    idle = first_prep - c_first
    gap = nb[0] - b[1]
    steady = gap < 1000.0 and n > 0  # (the first pair follows the warm-up; passes B more than 1 ms apart are the bench's checks)
    out.append(f"| {n}{'' if steady else ' (not counted)'} | {b[1] - b[0]:.1f} | {c_first - b[1]:.1f} | {tail_c:.1f} | "
               f"{', '.join(f'{e[1] - e[0]:.1f}' for e in cs)} | {idle:.1f} | {prep_us:.1f} | {a_us:.1f} | {kth_us:.1f} | {nb[0] - first_prep:.1f} | {gap:.1f} |")
    if not steady:
        continue
    agg["first_c"].append(c_first - b[1])
    agg["tail_c"].append(tail_c)
    agg["prelude"].append(nb[0] - first_prep)
    agg["idle"].append(idle)
    agg["gap"].append(gap)
    agg["b"].append(b[1] - b[0])
if agg["gap"]:
    med = {k: statistics.median(v) for k, v in agg.items()}
    out.append("")
    out.append(f"median over {len(agg['gap'])} pairs: pass B {med['b']:.1f} us, B end -> first C end {med['first_c']:.1f} us, "
               f"B end -> last C end {med['tail_c']:.1f} us, idle from the first C end to the next prep {med['idle']:.1f} us, "
               f"prep -> next B start {med['prelude']:.1f} us, B end -> next B start {med['gap']:.1f} us")
text = "\n".join(out) + "\n"
if len(sys.argv) > 2 and sys.argv[2] != "-":
    open(sys.argv[2], "w").write(text)
print(text)
