// pvs_rrf_batch.hip — C ABI of libpvs: pvs_rrf_search_batch, the PQL `or` arm for a batch of composed queries.  pvs_rrf_search
// streams every byte of every branch for ONE composed query; here each branch is scored for up to 32 queries of the batch in one
// corpus pass (the per-item scorers of pvs_search_groups), the window keys of the whole chunk come out of one launch per branch, and
// the first round of the bounded fusion runs for the whole chunk at once on the device (rrf_round_device, the single call's round
// with nq = the chunk: one launch per step, one synchronisation); each query then continues, where it must, over its own columns with the single-query fusion (pvs_rrf_search.hip) — so every page
// is pvs_rrf_search's, bit for bit, without re-scoring the corpus.
#include "pvs_rrf_search.hpp"

namespace {
constexpr uint32_t RRF_BATCH_CHUNK = 32;  // queries per corpus pass (the fused scorer's MODE 3 tile of 32 query lanes)

// One branch scored for a chunk of queries: per query j, the aggregates vals[j * n_groups ...] and window keys keys[j * n_groups ...]
struct BranchChunk {
    double *vals = nullptr;              // [nq][n_groups]
    unsigned long long *keys = nullptr;  // [nq][n_groups]
};

// device bytes one chunk of nq queries holds for branch b at its peak
uint64_t chunk_bytes(const pvs_rrf_branch &b, uint32_t nq) {
    const pvs_index *ix = b.idx;
    if (ix->n == 0) return 0;
    const uint64_t G = std::max<uint32_t>(ix->n_groups, 1);
    const bool fused = fused_groups_ok(ix, nq, nullptr, nullptr);
    return (uint64_t)ix->n * nq * 4 + G * nq * 8 * (fused ? 3 : 2) + (uint64_t)ix->dim * 4 * nq + (b.row_weights ? ix->n * 4 : 0);
}

// Queries [q0, q0 + nq) of branch b: one corpus pass, the aggregates of every group, the window keys.  Complete (synchronised) on return.
pvs_status score_branch_chunk(const pvs_rrf_branch &b, uint32_t q0, uint32_t nq, BranchChunk *out) {
    pvs_index *ix = b.idx;
    if (ix->n == 0) return PVS_OK;
    if (ix->n > (1ull << 31) / 4) return pvs_fail(PVS_ERR_UNSUPPORTED, "more than 2^29 rows in one dense column");
    HIP_TRY(hipSetDevice(ix->device));
    const uint32_t G = ix->n_groups;
    uint32_t t;
    SearchCtx *c = ctx_acquire(ix, &t);
    void *d_q = nullptr;
    float *d_m = nullptr, *d_w = nullptr;
    double *d_vt = nullptr;
    auto body = [&]() -> pvs_status {
        PVS_TRY(ctx_prepare(ix, *c, nq, 1, false));
        PVS_TRY(ctx_pinned_io(*c, 64));  // (word 8: the fused scorer's out-of-range flag)
        const size_t qbytes = (size_t)ix->dim * (b.query_dtype == PVS_I8 ? 1 : 4);
        HIP_TRY(pvs_scratch_alloc(&d_q, qbytes * nq));
        HIP_TRY(hipMemcpyAsync(d_q, (const uint8_t *)b.query + qbytes * q0, qbytes * nq, hipMemcpyHostToDevice, c->stream));
        if (b.row_weights) {
            HIP_TRY(pvs_scratch_alloc((void **)&d_w, ix->n * 4));
            HIP_TRY(hipMemcpyAsync(d_w, b.row_weights, ix->n * 4, hipMemcpyHostToDevice, c->stream));
        }
        HIP_TRY(pvs_scratch_alloc((void **)&d_m, (size_t)ix->n * nq * 4));
        HIP_TRY(pvs_scratch_alloc((void **)&out->vals, (size_t)std::max<uint32_t>(G, 1) * nq * 8));
        HIP_TRY(pvs_scratch_alloc((void **)&out->keys, (size_t)std::max<uint32_t>(G, 1) * nq * 8));
        const uint32_t pad = nq <= 32 ? 32 : nq <= 64 ? 64 : 128;
        PVS_TRY(prep_chunk(ix, *c, d_q, b.query_dtype, 0, nq, pad, b.metric));
        const int desc = b.row_n_descending != 0;
        bool inorder = false;
        if (fused_groups_ok(ix, nq, nullptr, d_w)) {
            // one pass: every group's aggregate, group-major [G][nq] -> per-query keys and values (one transposing launch)
            HIP_TRY(pvs_scratch_alloc((void **)&d_vt, (size_t)std::max<uint32_t>(G, 1) * nq * 8));
            PVS_TRY(fused_group_chunk(ix, *c, nq, pad, b.metric, b.agg, d_w, nullptr, d_m, d_vt));
            HIP_TRY(hipStreamSynchronize(c->stream));
            if (*(volatile uint32_t *)(c->h_io + 32) == 0) return pvs_rrf_window_keys_t(d_vt, G, nq, desc, out->keys, out->vals, c->stream);
            // an L2 sum left the closed form's range: every row again, in order (as dense_chunk does for one query).  The flag is one
            // word for the chunk, so every query of it is scored again, not only the one that left the range: correct, and rare on
            // real embeddings (their int8 codes stay far from the +-127 corners the 2^24 bound assumes)
            inorder = true;
        }
        PVS_TRY(dense_chunk(ix, *c, nq, pad, b.metric, d_m, nullptr, inorder));
        // column-major [nq][G] aggregates straight from the matrix; the keys are elementwise over all columns
        HIP_TRY(pvs_launch_group_aggregate(d_m, nq, nq, 0, ix->d_grp_off, ix->d_grp_rows, G, d_w, nullptr, b.agg, out->vals, c->stream));
        if ((uint64_t)G * nq <= 0x7fffffffull) return pvs_rrf_window_keys(out->vals, G * nq, desc, out->keys, c->stream);
        for (uint32_t j = 0; j < nq; j++) PVS_TRY(pvs_rrf_window_keys(out->vals + (size_t)j * G, G, desc, out->keys + (size_t)j * G, c->stream));
        return PVS_OK;
    };
    pvs_status st = body();
    // the fusion reads the columns from other streams: they are complete before the call returns
    hipError_t e = hipStreamSynchronize(c->stream);
    if (st == PVS_OK && e != hipSuccess) st = pvs_fail(PVS_ERR_DEVICE, "scoring a branch: %s", hipGetErrorString(e));
    for (void *p : {d_q, (void *)d_m, (void *)d_w, (void *)d_vt}) pvs_scratch_free_on(p, c->stream);
    ix->searches++;
    ix->dense_queries += nq;
    ctx_done(ix, c);
    return st;
}

void free_chunk(std::vector<BranchChunk> &ch) {
    for (auto &c : ch) {
        pvs_scratch_free(c.vals);
        pvs_scratch_free(c.keys);
        c = BranchChunk();
    }
}

// queries per chunk: <= 32, the [n][nq] matrix of every branch <= 2 GiB (dense_chunk_queries), and every branch's chunk in free memory
uint32_t first_chunk(const pvs_rrf_branch *br, uint32_t nb, uint32_t batch) {
    uint32_t cq = std::min(batch, RRF_BATCH_CHUNK);
    for (uint32_t b = 0; b < nb; b++) cq = std::min(cq, dense_chunk_queries(br[b].idx, cq));
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return cq;
    const uint64_t budget = (uint64_t)((double)free_b * 0.85);
    auto need = [&](uint32_t q) {
        uint64_t s = 0;
        for (uint32_t b = 0; b < nb; b++) s += chunk_bytes(br[b], q);
        return s;
    };
    while (cq > 1 && need(cq) > budget) cq--;
    return cq;
}
}  // namespace

// Row j of the outputs = pvs_rrf_search with every branch's query set to its j-th vector (see pvs.h)
PVS_EXPORT pvs_status pvs_rrf_search_batch(const pvs_rrf_branch *br, uint32_t nb, uint32_t batch, uint32_t k, int64_t *out_groups,
                                           double *out_scores, uint32_t *out_counts) {
    const uint32_t nb_ok = br && nb <= (uint32_t)PVS_RRF_MAX_BRANCHES ? nb : 0;
    // (pvs_gate.hip: every branch's index shared for the whole call — every chunk of the batch sees one state of every index)
    GateSharedMany gate(br, br + nb_ok, [](const pvs_rrf_branch &b) { return b.idx; });
    if (!br || !out_groups || !out_scores || !out_counts) return pvs_fail(PVS_ERR_INVALID_ARG, "null argument");
    if (nb < 1 || nb > (uint32_t)PVS_RRF_MAX_BRANCHES) return pvs_fail(PVS_ERR_INVALID_ARG, "1..%d branches", PVS_RRF_MAX_BRANCHES);
    if (k < 1) return pvs_fail(PVS_ERR_INVALID_ARG, "k must be a positive integer");
    bool multi = false;
    PVS_TRY(rrf_check_multi(br, nb, &multi));  // (the single call's checks and statuses)
    std::vector<pvs_rrf_branch> one(br, br + nb);  // the branches with query j
    auto query_of = [&](uint32_t b, uint32_t j) {
        const size_t qbytes = (size_t)br[b].idx->dim * (br[b].query_dtype == PVS_I8 ? 1 : 4);
        return (const void *)((const uint8_t *)br[b].query + qbytes * j);
    };
    if (multi) {
        // multi-device branches: one composed query after the other (correct, not faster than pvs_rrf_search)
        if (batch == 0) return PVS_OK;
        int32_t path = 0;
        for (uint32_t j = 0; j < batch; j++) {
            for (uint32_t b = 0; b < nb; b++) one[b].query = query_of(b, j);
            PVS_TRY(rrf_search_one(one.data(), nb, k, out_groups + (size_t)j * k, out_scores + (size_t)j * k, out_counts + j));
            path = std::max(path, pvs_rrf_last_path());
        }
        rrf_set_last_path(path);
        return PVS_OK;
    }
    PvsRrfParams p;
    PVS_TRY(rrf_check_branches(br, nb, &p));
    if (batch == 0) return PVS_OK;
    const bool keyed = rrf_branches_keyed(br, nb);
    std::vector<BranchChunk> ch(nb);
    int32_t path = 0;
    auto body = [&]() -> pvs_status {
        uint32_t cq = first_chunk(br, nb, batch);
        for (uint32_t q0 = 0; q0 < batch;) {
            const uint32_t nq = std::min(cq, batch - q0);
            pvs_status st = per_branch(br, nb, [&](uint32_t b) { return score_branch_chunk(br[b], q0, nq, &ch[b]); });
            if (st != PVS_OK) {
                (void)hipDeviceSynchronize();
                free_chunk(ch);
                if (st == PVS_ERR_OOM && cq > 1) {  // the estimate was optimistic: a smaller chunk
                    cq = std::max<uint32_t>(1, cq / 2);
                    continue;
                }
                return st;
            }
            // Round 0 of every query at once on the device where the single call would run it there; then each query continues on its
            // own columns as the single call would (the columns stay put: no re-scoring, whatever the fusion needs).  Order keys ask
            // for pages longer than k: those queries take the single-query fusion whole.
            std::vector<uint8_t> state;
            uint64_t target = 0;
            if (!keyed) {
                std::vector<RrfBranchCols> shape(nb);
                for (uint32_t b = 0; b < nb; b++) shape[b].n_groups = br[b].idx->n_groups;
                target = rrf_device_round_target(shape, p, k);
            }
            if (target) {
                std::vector<const unsigned long long *> keys((size_t)nq * nb);
                for (uint32_t j = 0; j < nq; j++)
                    for (uint32_t b = 0; b < nb; b++) keys[(size_t)j * nb + b] = ch[b].keys ? ch[b].keys + (size_t)j * br[b].idx->n_groups : nullptr;
                state.resize(nq);
                PVS_TRY(rrf_round_device(br, nb, keys.data(), nq, p, target, k, out_groups + (size_t)q0 * k, out_scores + (size_t)q0 * k, out_counts + q0,
                                         state.data(), nullptr));
            }
            for (uint32_t j = 0; j < nq; j++) {
                std::vector<RrfBranchCols> cols(nb);
                for (uint32_t b = 0; b < nb; b++) {
                    const uint32_t G = br[b].idx->n_groups;
                    cols[b].ix = br[b].idx;
                    cols[b].n_groups = G;
                    cols[b].d_vals = ch[b].vals ? ch[b].vals + (size_t)j * G : nullptr;
                    cols[b].d_keys = ch[b].keys ? ch[b].keys + (size_t)j * G : nullptr;
                    one[b].query = query_of(b, q0 + j);
                }
                const size_t q = q0 + j;
                int qpath = 0;
                if (target && state[j] == 2) {
                    qpath = 1;
                } else if (target) {
                    PVS_TRY(rrf_fuse_continue(one.data(), cols, p, k, out_groups + q * k, out_scores + q * k, out_counts + q, &qpath, state[j] ? 1 : 0,
                                              state[j] == 0 ? false : true));
                } else if (!keyed) {
                    PVS_TRY(rrf_fuse_scored(one.data(), cols, p, k, out_groups + q * k, out_scores + q * k, out_counts + q, &qpath));
                } else {
                    PVS_TRY(rrf_keyed_page(
                        one.data(), nb, k,
                        [&](uint32_t kk, int64_t *g, double *sc, uint32_t *cnt) {
                            for (auto &c : cols) c.sample.clear();
                            return rrf_fuse_scored(one.data(), cols, p, kk, g, sc, cnt, &qpath);
                        },
                        out_groups + q * k, out_scores + q * k, out_counts + q));
                }
                path = std::max(path, (int32_t)qpath);
            }
            free_chunk(ch);
            q0 += nq;
        }
        return PVS_OK;
    };
    pvs_status st = body();
    if (st != PVS_OK) (void)hipDeviceSynchronize();
    free_chunk(ch);
    if (st == PVS_OK) rrf_set_last_path(path);
    return st;
}
