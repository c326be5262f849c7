// pvs_rrf_search.hpp — the pieces of pvs_rrf_search (pvs_rrf_search.hip) that its batched form (pvs_rrf_batch.hip) shares: the
// scored columns of a branch, the per-branch threads, round 0 of the bounded fusion on the device for nq >= 1 queries, the fusion of
// scored branches and the order-key page.
#pragma once
#include <functional>
#include <string>
#include <thread>
#include <vector>

#include "pvs_index.hpp"

// One branch of an OR-composition, scored (pvs_rrf_cols in the C ABI): every group's aggregate (f64, the reference's
// arithmetic) and its window key.
struct pvs_rrf_cols {
    pvs_index *ix = nullptr;
    double *d_vals = nullptr;               // [n_groups]
    unsigned long long *d_keys = nullptr;   // [n_groups] order-preserving window key (NULL placement and direction folded in)
    uint32_t n_groups = 0;
    std::vector<unsigned long long> sample;  // sorted sample of the keys (threshold proposals)
};
typedef pvs_rrf_cols RrfBranchCols;

// The branches of a composition live in different indexes (their own streams, contexts and scratch): their per-branch steps run
// on one host thread each, so that the round trips of one branch (uploads, the exact-range flag, page and count read-backs)
// hide behind the other's kernels.  Branches that share an index run one after the other.
template <class F>
inline pvs_status per_branch(const pvs_rrf_branch *br, uint32_t nb, F &&f) {
    bool distinct = true;
    for (uint32_t a = 0; a < nb; a++)
        for (uint32_t b = a + 1; b < nb; b++) distinct &= br[a].idx != br[b].idx;
    const bool serial = pvs_dbg(PVS_DBG_RRF_SERIAL) != 0;  // tuning
    if (nb == 1 || !distinct || serial) {
        for (uint32_t b = 0; b < nb; b++) PVS_TRY(f(b));
        return PVS_OK;
    }
    std::vector<pvs_status> st(nb, PVS_OK);
    std::vector<std::string> msg(nb);
    std::vector<std::thread> th;
    for (uint32_t b = 1; b < nb; b++)
        th.emplace_back([&, b] {
            st[b] = f(b);
            if (st[b] != PVS_OK) msg[b] = pvs_last_error();
        });
    st[0] = f(0);
    for (auto &t : th) t.join();
    if (st[0] != PVS_OK) return st[0];
    for (uint32_t b = 1; b < nb; b++)
        if (st[b] != PVS_OK) return pvs_fail(st[b], "%s", msg[b].c_str());
    return PVS_OK;
}

// The multi-device dispatch's checks (pvs_rrf_search's): *multi = the branches go to multi_rrf_search
pvs_status rrf_check_multi(const pvs_rrf_branch *br, uint32_t nb, bool *multi);
// Checks every single-device branch as pvs_rrf_search does (query, metric, one device, aggregation), builds the indexes' groups and
// fills p.  Multi-device branches are the caller's business.
pvs_status rrf_check_branches(const pvs_rrf_branch *br, uint32_t nb, PvsRrfParams *p);
// The fused page of scored branches: the bounded fusion, else every group of every branch ranked.  *path = 1 / 2 (pvs_rrf_last_path).
// Slots past *out_count are written as -1 / NaN.  The columns are read, not freed.
pvs_status rrf_fuse_scored(const pvs_rrf_branch *br, std::vector<RrfBranchCols> &cols, const PvsRrfParams &p, uint32_t k, int64_t *out_groups,
                           double *out_scores, uint32_t *out_count, int *path);
// The same, continuing after a round 0 the caller ran on the device: first_round = 1 (the bound was not met) or first_round = 0 with
// device_round = false (a size limit of the device form was hit: round 0 in host form)
pvs_status rrf_fuse_continue(const pvs_rrf_branch *br, std::vector<RrfBranchCols> &cols, const PvsRrfParams &p, uint32_t k, int64_t *out_groups,
                             double *out_scores, uint32_t *out_count, int *path, int first_round, bool device_round);
// Round 0 of the bounded fusion for nq queries on the device (pvs_rrf_round_device): every step one launch for all of them, one
// synchronisation.  keys[j * nb + b]: query j's window keys in branch b.  state[j]: 2 = the bound was met and query j's page is
// written (out_*: [nq][k], out_counts[j]), 1 = not met (the query continues at round 1), 0 = a size limit of the device form was hit
// (the host form redoes round 0).  out_m (may be null): each query's candidates.
pvs_status rrf_round_device(const pvs_rrf_branch *br, uint32_t nb, const unsigned long long *const *keys, uint32_t nq, const PvsRrfParams &p,
                            uint64_t target, uint32_t k, int64_t *out_groups, double *out_scores, uint32_t *out_counts, uint8_t *state, uint32_t *out_m);
// The page target of round 0 when rrf_fuse_scored would run that round on the device (rrf_round_device), else 0
uint64_t rrf_device_round_target(const std::vector<RrfBranchCols> &cols, const PvsRrfParams &p, uint32_t k);
// true when a branch's rows carry order keys (pvs_index_set_order_keys): the page then goes through rrf_keyed_page
bool rrf_branches_keyed(const pvs_rrf_branch *br, uint32_t nb);
// The page under the order-key tie rule: `page(kk, ...)` answers the plain fused page of kk slots; it is asked for pages longer than k
// until every group tying with the k-th score is on one, which is then re-ordered by key DESC and cut to k.
pvs_status rrf_keyed_page(const pvs_rrf_branch *br, uint32_t nb, uint32_t k,
                          const std::function<pvs_status(uint32_t kk, int64_t *g, double *sc, uint32_t *cnt)> &page, int64_t *out_groups,
                          double *out_scores, uint32_t *out_count);
// pvs_rrf_search without the gate (the caller holds every branch's index shared)
pvs_status rrf_search_one(const pvs_rrf_branch *br, uint32_t nb, uint32_t k, int64_t *out_groups, double *out_scores, uint32_t *out_count);
// pvs_rrf_last_path of this thread
void rrf_set_last_path(int32_t path);
