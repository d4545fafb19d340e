// api_vr.hip -- the variance-reduction (ALC) criterion: the utility of a candidate is how much its static reading lowers
// the summed predictive variance of the targets T (the ordinary rows of the candidate set, fixed by the solve), see
// include/algp_hip.h.  With the signed cross term E_jc = [c ordinary] C(j, c) - (V V^T)_jc, the target weights omega (one per
// pool site, algp_set_target_weights; 1 where none are attached) and w_c = sum_{j in T} omega_j E_jc^2,
//   u_c = w_c / (pv_c + ss) (ordinary c)        u_c = -delta w_c / (1 + delta s_cc) (unit c),
// so the state is the vector w (VrState, common.h); new weights drop it.
//   First scoring after a solve (vr_product): w is the row sums of the squared M x M matrix E over its target columns -- one
//     fused product V^T V on the matrix cores whose epilogue forms E in registers and leaves one partial sum per row and
//     128-column tile (gemm.hip: gemm_nt_launch_vr); neither E nor a kernel-matrix block is written.  The column tiles go in
//     chunks of VR_CHUNK so that the partial sums stay small, and are added in tile order (vr_combine_kernel).
//   Every later pick (vr_fold): its appended column r of V^T gives E' = E - r_T r_c^T, hence
//     w'_c = w_c - 2 r_c y_c + r_c^2 sum_T omega_j r_j^2 with rt = (omega r)_T and
//     y = E^T rt = kappa_c sum_{j in T} C(j, c) rt_j - V_c . (V_T^T rt):
//     a fused kernel-GEMV (or a row gather of an explicit covariance) and two passes over V^T instead of the product.
//   $ALGP_VR_RANK1=0 (cross-check): the full product at every scoring.
// Over the ranks of a communicator (algp_comm_set_vr_exchange): the targets are the ordinary rows of
// EVERY rank's shard (the shards disjoint), and a rank keeps w for its own rows only.  The targets of the other ranks enter
// through their rows of V^T and their pool indices -- the pool and the target weights are replicated:
//   agreement (first scoring of a call; comm_agree_checked, ten doubles): status, rows, picks committed and folded, whether this rank
//     needs a build and whether it builds at every scoring, the layout's rows per round, the weights' hash, Npad, n_pool;
//   build (vr_shard_build): a second four-double word (allocations), then R = ceil(largest shard / B) rounds -- pack rows
//     [tB, (t+1)B) behind their pool indices (vr_pack_rows_kernel), comm_exchange, ONE rectangular product of the rank's whole V^T
//     against the W B gathered rows (gemm_nt_launch_vrx), its partial sums added into w in the order round, rank, tile -- and a
//     last 32-byte exchange with the outcome of the disjointness check (vr_overlap_kernel);
//   fold (vr_shard_fold): ONE exchange per pick of every rank's partial t = V_T^T rt, partial sum_T omega r^2 and (pool index,
//     rt) pairs; the partials are summed in rank order, the kernel-GEMV runs over the gathered pairs for the rank's own rows.
// Every one of them carries each rank's status word (the protocol: above comm_first_failure in comm.hip).  The gather and
// the product of a round run one after the other on the context's stream.
#include "api_impl.h"

using namespace algp;

namespace algp {

constexpr int VR_CHUNK = 64;             // column tiles per launch of the product: 64 x Mpad partial sums

void release(algp_ctx* c, VrState& vr) {
    for (DevBuf* b : {&vr.W, &vr.Part, &vr.R, &vr.Tp, &vr.Tv, &vr.Y, &vr.Nrm, &vr.Obj, &vr.Mark, &vr.Tidx, &vr.Trt}) release(c, *b);
    vr.drop();
}

static bool lists_site_twice(const algp_ctx* c) {
    std::vector<int64_t> sorted(c->cand_idx);
    std::sort(sorted.begin(), sorted.end());
    return std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end();
}

// with q > 0 picks committed their columns [Npad, Npad + q) ride along in a product as one more 128-column k block: whatever
// else that block holds (columns no pick has written yet; the padding rows behind M, which never get a pick's entry) is
// zeroed first
template <typename T>
int Impl<T>::vr_zero_picks_block(algp_ctx* c, int64_t q) {
    const int64_t M = c->M, Mpad = c->Mpad, Npad = c->Npad, ldv = c->ldv;
    if (q <= 0) return ALGP_OK;
    if (q < NB)
        ALGP_HIP(hipMemset2DAsync(p(c->Vt) + Npad + q, sizeof(T) * ldv, 0, sizeof(T) * (NB - q), Mpad, c->stream));
    if (Mpad > M)
        ALGP_HIP(hipMemset2DAsync(p(c->Vt) + M * ldv + Npad, sizeof(T) * ldv, 0, sizeof(T) * NB, Mpad - M, c->stream));
    return ALGP_OK;
}

// w for the current state of V^T (all committed picks included), from scratch
template <typename T>
int Impl<T>::vr_product(algp_ctx* c) {
    VrState& vr = c->vr;
    vr.drop();
    vr.over_ranks = false;
    const int64_t M = c->M, Mpad = c->Mpad, Npad = c->Npad, ldv = c->ldv;
    const int64_t q = (int64_t)c->picks.size();
    const int64_t K = q > 0 ? Npad + NB : Npad;
    ALGP_TRY(vr_zero_picks_block(c, q));
    const int tiles = (int)(Mpad / NB);
    const int chunk = std::min(tiles, VR_CHUNK);
    ALGP_TRY(ensure(c, vr.W, sizeof(T) * Mpad));
    ALGP_TRY(ensure(c, vr.Part, sizeof(T) * (size_t)chunk * Mpad));
    const KmatSrc s = make_src(c);
    for (int t0 = 0; t0 < tiles; t0 += chunk) {
        const int nt = std::min(chunk, tiles - t0);
        ALGP_TRY(gemm_nt_launch_vr<T>(c, ALGP_PROF_GEMM_OTHER, Mpad, (int64_t)nt * NB, K, p(c->Vt), ldv, (int64_t)t0 * NB, s,
                                      (const int64_t*)c->Cidx.p, (const int*)c->ckind.p, M, c->has_tw ? (const T*)c->tw.p : nullptr,
                                      p(vr.Part), Mpad));
        ALGP_TRY(vr_combine_launch<T>(c, p(vr.Part), Mpad, nt, M, t0 > 0, p(vr.W)));
    }
    vr.npicks = q;
    vr.valid = true;
    return ALGP_OK;
}

// fold pick number q (0-based; its column of V^T is Npad + q, and E before it reads the columns left of that) into w
template <typename T>
int Impl<T>::vr_fold(algp_ctx* c, int64_t q) {
    VrState& vr = c->vr;
    const int64_t M = c->M, Mpad = c->Mpad, ldv = c->ldv;
    ALGP_TRY(ensure(c, vr.R, sizeof(T) * 2 * Mpad));
    ALGP_TRY(ensure(c, vr.Y, sizeof(T) * 2 * Mpad));
    ALGP_TRY(ensure(c, vr.Tp, sizeof(T) * (size_t)VR_TBLOCKS * ldv));
    ALGP_TRY(ensure(c, vr.Tv, sizeof(T) * ldv));
    ALGP_TRY(ensure(c, vr.Nrm, sizeof(T)));
    return vr_fold_launch<T>(c, M, (const int*)c->ckind.p, (const int64_t*)c->Cidx.p, p(c->Vt), ldv, c->Npad + q, make_src(c),
                             c->has_tw ? (const T*)c->tw.p : nullptr, p(vr.R), p(vr.R) + Mpad,
                             p(vr.Nrm), p(vr.Tp), p(vr.Tv), p(vr.Y), p(vr.Y) + Mpad, p(vr.W));
}

// utilities of every row into dst (device), stream-ordered; the rows are flushed (scores_enqueue)
template <typename T>
int Impl<T>::vr_scores_enqueue(algp_ctx* c, double ss, double delta, double* dst) {
    if (c->cextra.p)
        return fail(c, ALGP_ERR_STATE, "variance_reduction: candidates with an extra variance of their own are not supported");
    const bool rank1 = env_switch("ALGP_VR_RANK1", true);       // read per call: the tests flip it
    VrState& vr = c->vr;
    const int64_t q = (int64_t)c->picks.size();
    if (vr_over_ranks(c)) {
        // the state counts every rank's targets and only the collectives of vr_shard_step bring it up to date (algp_scores and
        // algp_greedy_sharded run them first): nothing here may score against this rank's own targets instead
        if (!(vr.valid && vr.over_ranks && vr.npicks == q))
            return fail(c, ALGP_ERR_STATE, "variance_reduction: this context scores the criterion over the ranks of its communicator "
                                           "(algp_comm_set_vr_exchange); call algp_scores or algp_greedy_sharded on every rank");
    } else if (c->M > 0) {
        if (!vr.valid || vr.over_ranks || !rank1 || vr.npicks > q) {
            // a pool site listed twice would be two targets with sigma_n^2 between them, which only the product sees (the fold
            // adds sigma_n^2 on a row's own entry alone): refused rather than scored two ways
            if (lists_site_twice(c))
                return fail(c, ALGP_ERR_STATE, "variance_reduction: the candidate set lists a pool site more than once");
            ALGP_TRY(vr_product(c));
        } else {
            while (vr.npicks < q) {
                const int rc = vr_fold(c, vr.npicks);
                if (rc != ALGP_OK) { vr.drop(); return rc; }
                ++vr.npicks;
            }
        }
    }
    return vr_score_launch<T>(c, c->M, (const int*)c->ckind.p, (const unsigned char*)c->alive.p, (const T*)c->dstat.p,
                              (const T*)vr.W.p, ss, delta, dst);
}

// ------------------------------------------------------------------ over the ranks of a communicator
// rows of V^T a rank contributes to each all-gather of the build: what the caller asked for, rounded up to a multiple of 128, or
// by default the largest multiple of 128 (at least 128) for which the (world + 1) slices [32-byte header | 8 bytes and
// Npad + 128 elements per row] of the staging buffer stay within 1 GiB (include/algp_hip.h)
static int64_t vr_rows_per_round(const algp_ctx* c) {
    if (c->vr.xrows > 0) return round_up(c->vr.xrows, NB);
    const int64_t per_rank = ((int64_t)1 << 30) / (c->comm_nranks + 1) - 32;
    const int64_t row_bytes = 8 + (int64_t)c->es * (c->Npad + MAX_APPEND);
    return std::max<int64_t>(per_rank / row_bytes / NB * NB, NB);
}

// bytes per rank of a fold's gather: [32-byte header | sum_T omega r^2 (16 bytes) | t over ldv columns | cap pool indices | cap
// values of rt], cap = the largest shard
static void vr_fold_layout(const algp_ctx* c, int64_t cap, int64_t* off_t, int64_t* off_idx, int64_t* off_val, size_t* bytes) {
    *off_t = 48;
    *off_idx = *off_t + round_up((int64_t)c->es * c->ldv, 16);
    *off_val = *off_idx + 8 * cap;
    *bytes = (size_t)round_up(*off_val + (int64_t)c->es * cap, 16);
}

// an agreed failure of a checked collective (comm.hip) drops the state: the next call rebuilds it
static const CommState VR_STATE = {"the variance-reduction state", [](algp_ctx* c) { c->vr.drop(); }};

// The build over the ranks: w of this rank's rows against the targets of every rank, all committed picks included.  Every
// rank has agreed to build (vr_shard_step); max_rows: the largest shard; st: this rank's status so far.
template <typename T>
int Impl<T>::vr_shard_build(algp_ctx* c, int64_t max_rows, int st) {
    VrState& vr = c->vr;
    vr.drop();
    const int nr = c->comm_nranks;
    const int64_t M = c->M, Mpad = c->Mpad, Npad = c->Npad, ldv = c->ldv;
    const int64_t q = (int64_t)c->picks.size();
    const int64_t K = q > 0 ? Npad + NB : Npad;
    const int64_t B = std::min(vr_rows_per_round(c), round_up(std::max<int64_t>(max_rows, 1), NB));
    const int64_t R = (max_rows + B - 1) / B;
    const size_t es = sizeof(T);
    const size_t slice = 32 + 8 * (size_t)B + es * (size_t)B * (size_t)K;
    const int tiles_round = (int)(B / NB) * nr;
    int64_t off_t, off_idx, off_val;
    size_t fbytes;
    vr_fold_layout(c, std::max<int64_t>(max_rows, 1), &off_t, &off_idx, &off_val, &fbytes);
    // every allocation of the build and of the folds behind it, then a word of its own: a rank that cannot hold the staging
    // buffer cannot take part in a gather through it
    int bst = st;
    if (bst == ALGP_OK && c->debug_fail_next_vr) {
        bst = fail(c, c->debug_fail_next_vr, "variance_reduction: failure injected by algp_debug_fail_at in the build over the ranks");
        c->debug_fail_next_vr = 0;
    }
    if (bst == ALGP_OK) bst = comm_rows_reserve(c, std::max(slice, fbytes));
    if (bst == ALGP_OK) bst = ensure(c, vr.Mark, sizeof(int) * (size_t)(c->n_pool + 1));
    if (bst == ALGP_OK && M > 0) {
        for (auto need : {std::make_pair(&vr.W, es * (size_t)Mpad), std::make_pair(&vr.Part, es * (size_t)tiles_round * (size_t)Mpad),
                          std::make_pair(&vr.R, es * 2 * (size_t)Mpad), std::make_pair(&vr.Y, es * 2 * (size_t)Mpad),
                          std::make_pair(&vr.Tp, es * (size_t)VR_TBLOCKS * (size_t)ldv)})
            if (bst == ALGP_OK) bst = ensure(c, *need.first, need.second);
    }
    for (auto need : {std::make_pair(&vr.Tv, es * (size_t)ldv), std::make_pair(&vr.Nrm, (size_t)16),
                      std::make_pair(&vr.Tidx, sizeof(int64_t) * (size_t)nr * (size_t)std::max<int64_t>(max_rows, 1)),
                      std::make_pair(&vr.Trt, es * (size_t)nr * (size_t)std::max<int64_t>(max_rows, 1))})
        if (bst == ALGP_OK) bst = ensure(c, *need.first, need.second);
    {
        const double mine[4] = {(double)bst, 0.0, 0.0, 0.0};
        std::vector<double> all;
        ALGP_TRY(comm_agree_checked(c, VR_STATE, "the allocations of the build", mine, all));
    }
    int lst = ALGP_OK;                                          // what a launch of this rank failed with: its status in the next exchange
    if (M > 0) lst = vr_zero_picks_block(c, q);
    if (lst == ALGP_OK) lst = vr_mark_launch(c, M, (const int64_t*)c->Cidx.p, c->n_pool, (int*)vr.Mark.p);
    char* own = (char*)c->rowx.p;
    const char* all = own + slice;
    const KmatSrc s = make_src(c);
    for (int64_t t = 0; t < R; ++t) {
        if (lst == ALGP_OK)
            lst = vr_pack_rows_launch<T>(c, M, t * B, B, (const int*)c->ckind.p, (const int64_t*)c->Cidx.p, p(c->Vt), ldv, K, Npad + q,
                                         (int64_t*)(own + 32), (T*)(own + 32 + 8 * B));
        ALGP_TRY(comm_exchange(c, VR_STATE, "a round of the build", slice, lst));
        lst = vr_overlap_launch(c, all + 32, (int64_t)slice, nr, c->comm_rank, B, c->n_pool, (int*)vr.Mark.p);
        if (lst == ALGP_OK && M > 0)
            lst = gemm_nt_launch_vrx<T>(c, ALGP_PROF_GEMM_OTHER, Mpad, B, K, p(c->Vt), ldv, (const T*)(all + 32 + 8 * B), K,
                                        (const int64_t*)(all + 32), nr, (int64_t)slice, s, (const int64_t*)c->Cidx.p,
                                        (const int*)c->ckind.p, M, c->has_tw ? (const T*)c->tw.p : nullptr, p(vr.Part), Mpad);
        if (lst == ALGP_OK && M > 0) lst = vr_combine_launch<T>(c, p(vr.Part), Mpad, tiles_round, M, t > 0, p(vr.W));
    }
    // the outcome: a pool site that two ranks list is seen by both of them, and every rank returns the refusal
    int hit = 0;
    if (lst == ALGP_OK && hipMemcpyAsync(&hit, (const int*)vr.Mark.p + c->n_pool, sizeof(int), hipMemcpyDeviceToHost, c->stream) != hipSuccess)
        lst = fail(c, ALGP_ERR_HIP, "variance_reduction: reading the disjointness check back failed");
    if (lst == ALGP_OK) lst = sync_checked(c, "variance_reduction (build over the ranks)");
    if (lst == ALGP_OK && hit)
        lst = fail(c, ALGP_ERR_STATE, "variance_reduction: a pool site of this rank's candidate set is listed by another rank too; the "
                                      "shards must be disjoint");
    ALGP_TRY(comm_exchange(c, VR_STATE, "the build", 32, lst));
    vr.npicks = q;
    vr.max_rows = max_rows;
    vr.over_ranks = true;
    vr.valid = true;
    return ALGP_OK;
}

// fold the next committed pick (q = vr.npicks) into w on every rank: one gather, see the top of the file
template <typename T>
int Impl<T>::vr_shard_fold(algp_ctx* c, int st) {
    VrState& vr = c->vr;
    const int nr = c->comm_nranks;
    const int64_t M = c->M, Mpad = c->Mpad, ldv = c->ldv;
    const int64_t q = vr.npicks, col = c->Npad + q, cap = std::max<int64_t>(vr.max_rows, 1);
    int64_t off_t, off_idx, off_val;
    size_t bytes;
    vr_fold_layout(c, cap, &off_t, &off_idx, &off_val, &bytes);
    st = comm_fold_status(c, st, vr.valid && vr.over_ranks, "the variance-reduction state over the ranks", q, "variance_reduction",
                          &c->debug_fail_next_vr);
    if (c->rowx.cap < bytes * (size_t)(nr + 1) || (c->host_gather && c->rowx_host_cap < bytes * (size_t)(nr + 1))) {
        // the build and vr_shard_step reserve the staging before a word that carries their failure, so this is a rank that never
        // built: its refusal (set above) or the reservation's travels in the status word like any other -- unless no buffer is
        // left to carry a word in, which returns here as a failing transport does
        const int rr = comm_rows_reserve(c, bytes);
        if (st == ALGP_OK) st = rr;
        if (rr != ALGP_OK && (c->rowx.cap < bytes * (size_t)(nr + 1) || (c->host_gather && c->rowx_host_cap < bytes * (size_t)(nr + 1))))
            return rr;
    }
    char* own = (char*)c->rowx.p;
    const T* tw = c->has_tw ? (const T*)c->tw.p : nullptr;
    if (st == ALGP_OK && hipMemsetAsync(own, 0, bytes, c->stream) != hipSuccess)
        st = fail(c, ALGP_ERR_HIP, "variance_reduction: clearing this rank's share of a fold failed");
    // 1. this rank's share of the two sums over the targets, and its targets' (pool index, rt) pairs
    if (st == ALGP_OK)
        st = vr_fold_local_launch<T>(c, M, (const int*)c->ckind.p, (const int64_t*)c->Cidx.p, p(c->Vt), ldv, col, tw, p(vr.R), p(vr.R) + Mpad,
                                     (T*)(own + 32), p(vr.Tp), (T*)(own + off_t));
    if (st == ALGP_OK)
        st = vr_pairs_launch<T>(c, M, cap, (const int*)c->ckind.p, (const int64_t*)c->Cidx.p, M > 0 ? p(vr.R) + Mpad : (const T*)nullptr,
                                (int64_t*)(own + off_idx), (T*)(own + off_val));
    ALGP_TRY(comm_exchange(c, VR_STATE, "the fold of a pick", bytes, st));
    // 2. the sums in rank order, the kernel-GEMV over every rank's pairs for this rank's rows, the update of w
    const int rc = [&]() {
        ALGP_TRY(vr_fold_gathered_launch<T>(c, own + bytes, (int64_t)bytes, nr, col, cap, 32, off_t, off_idx, off_val, p(vr.Tv), p(vr.Nrm),
                                            (int64_t*)vr.Tidx.p, p(vr.Trt)));
        return vr_fold_apply_launch<T>(c, M, (const int*)c->ckind.p, (const int64_t*)c->Cidx.p, p(c->Vt), ldv, col, make_src(c),
                                       (int64_t)nr * cap, (const int64_t*)vr.Tidx.p,
                                       (const T*)vr.Trt.p, (const T*)vr.R.p, (const T*)vr.R.p + Mpad, (const T*)vr.Nrm.p, (const T*)vr.Tv.p,
                                       p(vr.Y), p(vr.Y) + Mpad, p(vr.W));
    }();
    if (rc != ALGP_OK) { vr.drop(); return rc; }
    vr.npicks += 1;
    return ALGP_OK;
}

// Bring the state over the ranks up to the committed picks, on every rank together.  st: this rank's status so far (it still
// takes part in every collective).  first_of_call: the first scoring of an ABI call -- the agreement word decides whether
// every rank (re)builds; later picks of an algp_greedy_sharded call fold the one pick committed since (or, where a rank
// runs with ALGP_VR_RANK1=0, build again: the word says so to everybody).
template <typename T>
int Impl<T>::vr_shard_step(algp_ctx* c, int st, bool first_of_call) {
    VrState& vr = c->vr;
    const int nr = c->comm_nranks;
    if (st == ALGP_OK && !c->solved) st = fail(c, ALGP_ERR_STATE, "scores: call algp_solve_candidates first");
    if (st == ALGP_OK && !c->prior_noise) st = fail(c, ALGP_ERR_STATE, "scores: candidates were set with predictive semantics");
    if (st == ALGP_OK && c->cextra.p)
        st = fail(c, ALGP_ERR_STATE, "variance_reduction: candidates with an extra variance of their own are not supported");
    if (st == ALGP_OK) st = flush_lazy(c);
    int64_t rounds = 1;
    if (first_of_call) {
        const bool rank1 = env_switch("ALGP_VR_RANK1", true);   // read per call: the tests flip it
        const int64_t q = (int64_t)c->picks.size();
        const bool have = vr.valid && vr.over_ranks;
        const bool need = !have || !rank1 || vr.npicks > q;
        // a pool site listed twice by this rank would be two targets with sigma_n^2 between them, which only the product sees
        if (st == ALGP_OK && need && lists_site_twice(c))
            st = fail(c, ALGP_ERR_STATE, "variance_reduction: the candidate set lists a pool site more than once");
        // the staging of the folds that follow a state this rank holds: reserved here, where the word below carries a failure
        if (st == ALGP_OK && have && !need) {
            int64_t off_t, off_idx, off_val;
            size_t fbytes;
            vr_fold_layout(c, std::max<int64_t>(vr.max_rows, 1), &off_t, &off_idx, &off_val, &fbytes);
            st = comm_rows_reserve(c, fbytes);
        }
        const uint64_t h = c->has_tw ? (c->tw_hash & (((uint64_t)1 << 52) - 1)) | 1 : 0;    // exact as a double; 0: no weights
        const double mine[10] = {(double)st, (double)c->M, (double)q, have ? (double)vr.npicks : 0.0, (need ? 1.0 : 0.0) + (rank1 ? 0.0 : 2.0),
                                 (double)vr.xrows, (double)h, (double)c->Npad, (double)c->n_pool, 0.0};
        std::vector<double> all;
        ALGP_TRY(comm_agree_checked(c, VR_STATE, "the plan", mine, all, 10));
        bool any_need = false, same_layout = true, same_tw = true, same_sizes = true;
        int64_t max_rows = 0;
        vr.every_time = false;                                  // read only by the later picks of a call that got past this word
        for (int r = 0; r < nr; ++r) {
            const double* a = &all[(size_t)r * 10];
            vr.every_time = vr.every_time || ((int)a[4] & 2) != 0;
            same_layout = same_layout && a[5] == mine[5];
            same_tw = same_tw && a[6] == mine[6];
            same_sizes = same_sizes && a[7] == mine[7] && a[8] == mine[8];
            max_rows = std::max(max_rows, (int64_t)a[1]);
        }
        if (!same_layout) {
            vr.drop();
            std::string got;
            for (int r = 0; r < nr; ++r) got += (r ? ", " : "") + std::to_string((int64_t)all[(size_t)r * 10 + 5]);
            return fail(c, ALGP_ERR_BAD_ARG, "variance_reduction: the ranks attached different layouts (rows per round per rank: " + got +
                                                 "); call algp_comm_set_vr_exchange with the same value on every rank");
        }
        if (!same_tw) {
            vr.drop();
            return fail(c, ALGP_ERR_BAD_ARG, "variance_reduction: the ranks hold different target weights; call algp_set_target_weights "
                                             "with the same weights on every rank");
        }
        if (!same_sizes) {
            vr.drop();
            return fail(c, ALGP_ERR_STATE, "variance_reduction: the ranks hold different pools or train sets");
        }
        ALGP_TRY(comm_picks_agree(c, VR_STATE, "variance_reduction", all, 10, 4, &any_need));
        if (any_need) ALGP_TRY(vr_shard_build(c, max_rows));
        rounds = q - vr.npicks;                                // the same on every rank (agreed above)
    } else if (vr.every_time) {
        ALGP_TRY(vr_shard_build(c, vr.max_rows, st));
        rounds = 0;
    }
    return comm_catch_up(c, rounds, st, &Impl<T>::vr_shard_fold);
}

// the pool's target weights (host doubles, checked by the caller; null: detach) to the device in the context's dtype
template <typename T>
int Impl<T>::set_target_weights(algp_ctx* c, const double* w) {
    if (w) {
        std::vector<T> h((size_t)c->n_pool);
        for (int64_t q = 0; q < c->n_pool; ++q) h[(size_t)q] = (T)w[q];
        ALGP_TRY(sync(c));                                      // nothing enqueued still reads the old weights
        ALGP_TRY(ensure(c, c->tw, sizeof(T) * (size_t)c->n_pool));
        ALGP_HIP(hipMemcpyAsync(c->tw.p, h.data(), sizeof(T) * (size_t)c->n_pool, hipMemcpyHostToDevice, c->stream));
        ALGP_TRY(sync(c));
    }
    c->has_tw = w != nullptr;
    c->tw_hash = 0;
    if (w) {
        // what ranks scoring together compare (vr_shard_step): FNV-1a over the weights as given
        uint64_t h = 1469598103934665603ull;
        for (int64_t q = 0; q < c->n_pool; ++q) {
            uint64_t bits;
            memcpy(&bits, &w[q], sizeof(bits));
            h = (h ^ bits) * 1099511628211ull;
        }
        c->tw_hash = h;
    }
    c->vr.drop();                                               // the next scoring is the full product, picks included
    return ALGP_OK;
}

// sum_{j in T} omega_j pv_j under the current state (committed picks included): one workgroup, a fixed order
template <typename T>
int Impl<T>::target_variance(algp_ctx* c, double* sum) {
    if (!c->solved) return fail(c, ALGP_ERR_STATE, "get_target_variance: call algp_solve_candidates first");
    if (c->cextra.p)
        return fail(c, ALGP_ERR_STATE, "get_target_variance: candidates with an extra variance of their own are not supported");
    if (lists_site_twice(c))
        return fail(c, ALGP_ERR_STATE, "get_target_variance: the candidate set lists a pool site more than once");
    ALGP_TRY(flush_lazy(c));
    ALGP_TRY(ensure(c, c->vr.Obj, sizeof(double)));
    ALGP_TRY(vr_target_sum_launch<T>(c, c->M, (const int*)c->ckind.p, (const int64_t*)c->Cidx.p, (const T*)c->dstat.p,
                                     c->has_tw ? (const T*)c->tw.p : nullptr, (double*)c->vr.Obj.p));
    ALGP_HIP(hipMemcpyAsync(sum, c->vr.Obj.p, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return sync(c);
}

template struct Impl<float>;
template struct Impl<double>;

}  // namespace algp

extern "C" {

int algp_set_target_weights(algp_ctx* c, const double* w, int64_t n_pool) {
    CHECK_CTX(c);
    if (c->n_pool <= 0) return fail(c, ALGP_ERR_STATE, "set_target_weights: set a pool first");
    if (w) {
        if (n_pool != c->n_pool)
            return fail(c, ALGP_ERR_BAD_ARG, "set_target_weights: " + std::to_string(n_pool) + " weights for a pool of " +
                                                 std::to_string(c->n_pool) + " sites");
        for (int64_t q = 0; q < n_pool; ++q)
            if (!(std::isfinite(w[q]) && w[q] >= 0.0))
                return fail(c, ALGP_ERR_BAD_ARG, "set_target_weights: weight " + std::to_string(q) + " is not finite and >= 0");
    }
    FINISH(c, DISPATCH(c, set_target_weights(c, w)));
}

int algp_comm_set_vr_exchange(algp_ctx* c, int64_t rows_per_round) {
    CHECK_CTX(c);
    if (rows_per_round == 0) {
        c->vr.drop_layout();
        return ALGP_OK;
    }
    if (!c->comm && !c->host_gather)
        return fail(c, ALGP_ERR_STATE, "comm_set_vr_exchange: call algp_comm_init (or algp_comm_init_host) first");
    if (rows_per_round < -1 || rows_per_round > ((int64_t)1 << 40))
        return fail(c, ALGP_ERR_BAD_ARG, "comm_set_vr_exchange: rows_per_round > 0, -1 (the default), or 0 (detach)");
    if (c->vr.xrows != rows_per_round) c->vr.drop();
    c->vr.xrows = rows_per_round;
    return ALGP_OK;
}

int algp_get_target_variance(algp_ctx* c, double* sum) {
    CHECK_CTX(c);
    if (!sum) return fail(c, ALGP_ERR_BAD_ARG, "get_target_variance: bad arguments");
    FINISH(c, DISPATCH(c, target_variance(c, sum)));
}

}  // extern "C"
