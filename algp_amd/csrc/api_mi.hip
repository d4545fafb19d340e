// api_mi.hip -- the mutual-information criterion (agent.py:330-339): H(A u i) + H(Abar \ i) - H(all_i) per candidate.  The
// last two terms need the diagonals of P = C_AbarAbar^-1 and Q = (C + D_all)^-1 over the WHOLE pool (mi_rank1_kernel,
// vecops.hip).  A build (once per candidate solve: the sets of mi_sets, the form's factorisations, mi_install) leaves
// X = L^-T (P = X X^T) resident in c->mi, which reads three things from it: diag(P)_i = |X_i,:|^2, a committed pick's column
// P_:,c = X X_c,:^T, and the rank-1 folds of mi_rank1_kernel (which need only that column and the earlier picks' columns),
// so a pick costs one O(n^2) pass over each X instead of two refactorisations.
// Form 0, one GPU (mi_build, mi_apply_pick): both X whole, each built, factored and inverted in its own buffer.
// Form 1, dealt over the ranks of a communicator (algp_comm_set_mi_groups), so that algp_greedy_sharded scores the MI
// criterion too.  Whoever holds a set of ROWS of X can compute those rows' diagonal entries and their entries of every later
// column; the only input from outside is row c itself.  Ranks [0, g_bar) hold the complement matrix and ranks [g_bar, world)
// the whole pool's (a world of one never comes here: greedy_picks keeps form 0 for it).  Inside a group every member builds
// and factors the group's matrix (replicated, no communication), computes only its own 128-row blocks of X (blocks member,
// member + g, ...: mi_trinv_rows, mi_shard.hip) and releases the factor.  The diagonals, the rank-1 lists U / W, their signs
// and the three entropies stay WHOLE on every rank, so scoring is mi_score_launch on each rank's own candidates.
// Collectives, all of them all-gathers through comm_agree_checked / comm_exchange (RCCL or the caller's host transport):
//   first pick of an algp_greedy_sharded call: a 32-byte agreement word (status, whether a build is needed, picks so far);
//     then, when any rank needs it, the build and ONE gather of every rank's diagonal pieces and entropies;
//   every pick folded: a gather of the owners' rows at the pick ([header | row of X_bar | row of X_all] per rank), then a
//     gather of every rank's entries of the pick's columns with the earlier terms removed; every rank puts the whole columns
//     together and folds them into its copy of both diagonals (mi_rank1_kernel, as on one GPU).
// Every one of them carries each rank's status word, so that a rank that fails keeps its peers company and every rank returns
// its code from the same call: the protocol is described once, above comm_first_failure in comm.hip.
#include "api_impl.h"

using namespace algp;

namespace algp {

void release(algp_ctx* c, MiState& mi) {
    for (DevBuf* b : {&mi.Xbar, &mi.Xall, &mi.DP, &mi.DQ, &mi.Pos, &mi.U, &mi.W, &mi.Col, &mi.H, &mi.Full, &mi.Fold}) release(c, *b);
    mi.valid = false;
}

// the sets of a build, from the train set (its noise read back) and the committed picks: A (sampled, with its noise), Abar
// (the others), all (every site, with its noise), posbar, and the padded sizes
template <typename T>
int Impl<T>::mi_sets(algp_ctx* c, double ss, double sm, MiPlan& pl) {
    const int64_t n = c->n_pool;
    if (c->train_has_repeats)
        return fail(c, ALGP_ERR_STATE, "mutual_information: the train set lists a site more than once; fuse its readings first");
    const double vf = 1.0 / (1.0 / ss + 1.0 / sm);
    std::vector<char> sampled(n, 0);
    std::vector<double> noise(n, 0.0);
    std::vector<T> trvar(c->Npad);
    ALGP_HIP(hipMemcpyAsync(trvar.data(), c->varA.p, sizeof(T) * c->Npad, hipMemcpyDeviceToHost, c->stream));
    ALGP_TRY(sync(c));
    for (int64_t a = 0; a < c->N; ++a) { sampled[c->train_idx[a]] = 1; noise[c->train_idx[a]] = (double)trvar[a]; }
    for (auto& pk : c->picks) {
        noise[pk.pool_idx] = sampled[pk.pool_idx] ? vf : ss;
        sampled[pk.pool_idx] = 1;
    }
    pl.posbar.assign(n, -1);
    pl.all.resize(n);
    pl.vall.resize(n);
    for (int64_t i = 0; i < n; ++i) {
        pl.all[i] = i;
        pl.vall[i] = (T)noise[i];
        if (sampled[i]) { pl.A.push_back(i); pl.vA.push_back((T)noise[i]); }
        else { pl.posbar[i] = (int64_t)pl.Abar.size(); pl.Abar.push_back(i); }
    }
    pl.mb = (int64_t)pl.Abar.size();
    pl.npad = round_up(std::max<int64_t>(n, 1), NB);
    pl.mbpad = round_up(std::max<int64_t>(pl.mb, 1), NB);
    return ALGP_OK;
}

// the state's whole vectors, on every form; col: the length of a pick's column buffer
template <typename T>
int Impl<T>::mi_vectors(algp_ctx* c, const MiPlan& pl, int64_t col) {
    ALGP_TRY(ensure(c, c->mi.DP, sizeof(T) * pl.mbpad));
    ALGP_TRY(ensure(c, c->mi.DQ, sizeof(T) * pl.npad));
    ALGP_TRY(ensure(c, c->mi.U, sizeof(T) * (size_t)MAX_APPEND * pl.mbpad));
    ALGP_TRY(ensure(c, c->mi.W, sizeof(T) * (size_t)MAX_APPEND * pl.npad));
    ALGP_TRY(ensure(c, c->mi.Col, sizeof(T) * col));
    ALGP_TRY(ensure(c, c->mi.Pos, sizeof(int64_t) * c->n_pool));
    return ensure(c, c->mi.H, sizeof(double) * (3 + 2 * MAX_APPEND));
}

// a finished build becomes the state: Hs = (H(A), H(Abar), H(all)) and posbar to the device, no pick folded in yet
template <typename T>
int Impl<T>::mi_install(algp_ctx* c, MiPlan& pl, const double* Hs, int form, double ss, double sm) {
    MiState& mi = c->mi;
    mi.posbar = std::move(pl.posbar);
    ALGP_HIP(hipMemcpyAsync(mi.H.p, Hs, 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    ALGP_HIP(hipMemcpyAsync(mi.Pos.p, mi.posbar.data(), sizeof(int64_t) * c->n_pool, hipMemcpyHostToDevice, c->stream));
    ALGP_TRY(sync(c));                                       // Hs and posbar are host memory
    mi.mb = pl.mb;
    mi.mbpad = pl.mbpad;
    mi.npad = pl.npad;
    mi.npicks = (int64_t)c->picks.size();
    mi.base = mi.npicks;
    mi.nbar = 0;
    mi.ss = ss;
    mi.sm = sm;
    mi.form = form;
    mi.valid = true;
    return ALGP_OK;
}

// ------------------------------------------------------------------ form 0: one GPU
template <typename T>
int Impl<T>::mi_build(algp_ctx* c, double ss, double sm) {
    c->mi.valid = false;
    MiPlan pl;
    ALGP_TRY(mi_sets(c, ss, sm, pl));
    const int64_t n = c->n_pool, mb = pl.mb, npad = pl.npad, mbpad = pl.mbpad;
    // Two pool-wide matrices stay resident -- each is built, factored and inverted IN its buffer (L in the strictly lower
    // tiles, X = L^-T on and above the diagonal: trinv_upper_inplace) -- say so with the byte count instead of failing
    // half-way through the allocations.  At config 4's own pool (110 000 sites, fp64) that is 2 x 96.8 GB (round 5 held a
    // third matrix, the factor being inverted: 290 GB) and 4 n^3 / 3 = 1.8e15 flop for the first pick.
    const size_t need = sizeof(T) * ((size_t)npad * npad + (size_t)mbpad * mbpad + (size_t)npad * NB +
                                     (size_t)MAX_APPEND * (npad + mbpad));
    const size_t held = c->auxInv.cap + c->mi.Xbar.cap + c->mi.Xall.cap + c->mi.U.cap + c->mi.W.cap;
    size_t free_b = 0, total_b = 0;
    ALGP_HIP(hipMemGetInfo(&free_b, &total_b));
    if (need > held + free_b)
        return fail(c, ALGP_ERR_OOM,
                    "mutual_information: the criterion keeps the triangular inverses of two pool-wide matrices resident: " +
                        std::to_string(need) + " bytes for n_pool = " + std::to_string(n) + ", " + std::to_string(held + free_b) +
                        " available; score this pool with the entropy criterion (it needs the candidates' rows only) or a smaller pool");
    double Hs[3] = {0.0, 0.0, 0.0};
    ALGP_TRY(set_entropy(c, pl.A.data(), (int64_t)pl.A.size(), pl.vA.data(), &Hs[0]));
    ALGP_TRY(ensure(c, c->mi.Xbar, sizeof(T) * mbpad * mbpad));
    ALGP_TRY(ensure(c, c->mi.Xall, sizeof(T) * npad * npad));
    ALGP_TRY(mi_vectors(c, pl, npad));
    for (int which = 0; which < 2; ++which) {
        const int64_t m = which ? n : mb, mpad = which ? npad : mbpad;
        if (!which && mb == 0) continue;
        T* X = p(which ? c->mi.Xall : c->mi.Xbar);
        // C_AbarAbar carries no measurement noise (agent.py:331), C + D_all every site's
        int64_t mp;
        ALGP_TRY(build_set_matrix(c, which ? pl.all.data() : pl.Abar.data(), m, which ? pl.vall.data() : nullptr, &mp, X));
        double ld = 0;
        ALGP_TRY(factor_resident(c, X, m, mpad, p(c->auxInv), SC_AUXLOGDET, SC_AUXINFO, &ld));
        Hs[1 + which] = (double)m * ENT_CONST + 0.5 * ld;
        ALGP_TRY(trinv_upper_inplace<T>(c, ALGP_PROF_GEMM_OTHER, X, mpad, mpad, p(c->auxInv)));
        ALGP_TRY(rows_reduce_launch<T>(c, X, m, mpad, mpad, (const T*)nullptr, p(which ? c->mi.DQ : c->mi.DP), (T*)nullptr, 0));
    }
    return mi_install(c, pl, Hs, 0, ss, sm);
}

// fold pick number q (committed after mi_build) into P, Q and the three entropies: stream-ordered, O(n^2)
template <typename T>
int Impl<T>::mi_apply_pick(algp_ctx* c, int64_t q, double ss, double sm) {
    MiState& mi = c->mi;
    const PickRec& pk = c->picks[(size_t)q];
    const int r = (int)(q - mi.base);                         // its slot in the rank-1 lists
    const double delta = 1.0 / (1.0 / ss + 1.0 / sm) - sm;
    double* Hs = (double*)mi.H.p;
    const LazyPick* lp = (const LazyPick*)c->lazypicks.p + q;
    const int64_t n = c->n_pool, npad = mi.npad, mbpad = mi.mbpad;
    if (!pk.in_train) {
        // the site leaves the complement: column of P = X X^T at its row, then the rank-1 removal
        const int64_t cb = mi.posbar[pk.pool_idx];
        if (cb < 0) return fail(c, ALGP_ERR_STATE, "mutual_information: a picked site is missing from the complement set");
        // column cb of P = X X^T: X's row cb is zero (the buffer holds L there) left of its own diagonal tile
        ALGP_TRY(rows_reduce_launch<T>(c, p(mi.Xbar), mi.mb, mbpad, mbpad, p(mi.Xbar) + cb * mbpad, (T*)nullptr, p(mi.Col),
                                       cb / NB * NB));
        ALGP_TRY(mi_rank1_launch<T>(c, mi.mb, p(mi.Col), p(mi.U), mbpad, Hs + 3, mi.nbar, cb, 0, 0.0, p(mi.DP), Hs + 1,
                                    (double*)nullptr, lp));
        mi.nbar += 1;
    }
    // its noise in C + D_all changes by ss (new site: 0 -> ss) or by v_fused - sm (mobile-sampled site)
    ALGP_TRY(rows_reduce_launch<T>(c, p(mi.Xall), n, npad, npad, p(mi.Xall) + pk.pool_idx * npad, (T*)nullptr, p(mi.Col),
                                   pk.pool_idx / NB * NB));
    ALGP_TRY(mi_rank1_launch<T>(c, n, p(mi.Col), p(mi.W), npad, Hs + 3 + MAX_APPEND, r, pk.pool_idx, 1, pk.in_train ? delta : ss,
                                p(mi.DQ), Hs + 2, Hs + 0, lp));
    return ALGP_OK;
}

template <typename T>
int Impl<T>::mi_scores_enqueue(algp_ctx* c, double ss, double sm, double delta, double* dst) {
    MiState& mi = c->mi;
    const int64_t np = (int64_t)c->picks.size();
    // a sharded state that is caught up scores as it is: its diagonals and entropies are whole on every rank; with picks
    // still to fold (they need its collectives) this GPU builds the whole inverses instead
    const bool sharded_current = mi.current(1, ss, sm, np) && mi.npicks == np;
    if (!sharded_current && !mi.current(0, ss, sm, np)) ALGP_TRY(mi_build(c, ss, sm));
    for (; mi.npicks < np; ++mi.npicks) ALGP_TRY(mi_apply_pick(c, mi.npicks, ss, sm));
    return mi_score_launch<T>(c, c->M, (const int*)c->ckind.p, (const int64_t*)c->Cidx.p, (const unsigned char*)c->alive.p,
                              (const T*)c->dstat.p, ss, delta, (const int64_t*)mi.Pos.p, (const T*)mi.DP.p,
                              (const T*)mi.DQ.p, (const double*)mi.H.p, dst);
}

// ------------------------------------------------------------------ form 1: dealt over the ranks
namespace {
// one matrix's group: ranks [first, first + g), this rank's place in it (member, -1: not in it), its row tiles
struct MiGroup {
    int first = 0, g = 1, member = -1;
    int64_t m = 0, mpad = 0, nloc = 0, maxloc = 0;    // nloc: this rank's 128-row tiles; maxloc: member 0's (the most)
};
}  // namespace

// which = 0: the complement matrix (m = its sites), 1: the whole pool's; a world of at least two, 1 <= mi.ncomp < world
static MiGroup mi_group(const algp_ctx* c, int which, int64_t m, int64_t mpad) {
    MiGroup G;
    G.first = which == 0 ? 0 : c->mi.ncomp;
    G.g = which == 0 ? c->mi.ncomp : c->comm_nranks - c->mi.ncomp;
    const int r = c->comm_rank - G.first;
    G.member = (r >= 0 && r < G.g) ? r : -1;
    G.m = m;
    G.mpad = mpad;
    const int64_t nt = m > 0 ? mpad / NB : 0;
    auto tiles = [&](int mem) { return nt > mem ? (nt - mem + G.g - 1) / G.g : (int64_t)0; };
    G.nloc = G.member >= 0 ? tiles(G.member) : 0;
    G.maxloc = tiles(0);
    return G;
}

// bytes per rank of the two gathers: a pick's rows [32-byte header | row of X_bar (mbpad) | row of X_all (npad)], and the
// pieces [header | complement pieces (maxloc x 128) | whole-pool pieces (maxloc x 128)] (the build's diagonals, a pick's columns)
static void mi_payloads(const algp_ctx* c, int64_t mb, int64_t mbpad, int64_t npad, size_t es, size_t* rbytes, size_t* cbytes) {
    const MiGroup Gb = mi_group(c, 0, mb, mbpad), Ga = mi_group(c, 1, c->n_pool, npad);
    *rbytes = 32 + es * (size_t)(mbpad + npad);
    *cbytes = 32 + es * (size_t)NB * (size_t)(Gb.maxloc + Ga.maxloc);
}

// an agreed failure of a checked collective (comm.hip) drops the state: the next call rebuilds it
static const CommState MI_STATE = {"the mutual-information state", [](algp_ctx* c) { c->mi.valid = false; }};

// host side of a build: the sets, the payload sizes, and this rank's memory check -- nothing allocated yet
template <typename T>
int Impl<T>::mi_shard_plan(algp_ctx* c, double ss, double sm, MiPlan& pl) {
    const int64_t n = c->n_pool;
    if (!c->solved) return fail(c, ALGP_ERR_STATE, "greedy: call algp_solve_candidates first");
    ALGP_TRY(mi_sets(c, ss, sm, pl));
    mi_payloads(c, pl.mb, pl.mbpad, pl.npad, sizeof(T), &pl.rbytes, &pl.cbytes);
    // Peak of this rank: the matrix it factors and inverts (the larger of its groups') + its row blocks of X + the whole
    // diagonals and rank-1 lists + the exchange's buffers.  At config 4's pool (110 000 sites, fp64) on 8 ranks split 4 + 4:
    // 96.9 GB + 24.2 GB; after the build the factor is released (24.5 GB of MI state per rank against 2 x 96.8 GB on one GPU;
    // the train factor, the candidate solve and set_entropy's scratch of the train set are held beside it, as on one GPU).
    const MiGroup Gb = mi_group(c, 0, pl.mb, pl.mbpad), Ga = mi_group(c, 1, n, pl.npad);
    const int64_t full = std::max(Gb.member >= 0 && pl.mb > 0 ? pl.mbpad : 0, Ga.member >= 0 ? pl.npad : 0);
    const size_t need = sizeof(T) * ((size_t)full * full + (size_t)full * NB + (size_t)Gb.nloc * NB * pl.mbpad +
                                     (size_t)Ga.nloc * NB * pl.npad + (size_t)(MAX_APPEND + 3) * (pl.npad + pl.mbpad)) +
                        std::max(pl.rbytes, pl.cbytes) * (size_t)(c->comm_nranks + 1) * 5 / 4;
    const size_t held = c->auxInv.cap + c->mi.Xbar.cap + c->mi.Xall.cap + c->mi.Full.cap + c->mi.U.cap + c->mi.W.cap + c->rowx.cap;
    size_t free_b = 0, total_b = 0;
    ALGP_HIP(hipMemGetInfo(&free_b, &total_b));
    if (need > held + free_b)
        return fail(c, ALGP_ERR_OOM,
                    "mutual_information (sharded): rank " + std::to_string(c->comm_rank) + " factors a " + std::to_string(full) +
                        "-row matrix and keeps " + std::to_string(Gb.nloc + Ga.nloc) + " row blocks of its inverse: " +
                        std::to_string(need) + " bytes for n_pool = " + std::to_string(n) + ", " + std::to_string(held + free_b) +
                        " available; put more ranks on that matrix (algp_comm_set_mi_groups), or score a smaller pool");
    return ALGP_OK;
}

// this rank's share of the build: H(A), its group's factor and entropy, its rows of X, their diagonal entries into its
// payload (rowx + 32 ...); H3 = (H(A), H(Abar), H(all)) as far as this rank knows them
template <typename T>
int Impl<T>::mi_shard_build(algp_ctx* c, MiPlan& pl, double* H3) {
    if (c->debug_fail_next_mi) {
        const int code = c->debug_fail_next_mi;
        c->debug_fail_next_mi = 0;
        return fail(c, code, "mutual_information: failure injected by algp_debug_fail_at in the sharded build");
    }
    const int64_t n = c->n_pool, mb = pl.mb, mbpad = pl.mbpad, npad = pl.npad;
    const MiGroup Gb = mi_group(c, 0, mb, mbpad), Ga = mi_group(c, 1, n, npad);
    const size_t es = sizeof(T);
    c->mi.valid = false;
    c->mi.form = 1;
    ALGP_TRY(sync(c));
    release(c, c->mi.Xbar);                                  // whole inverses of a one-GPU build, or another layout's rows
    release(c, c->mi.Xall);
    ALGP_TRY(set_entropy(c, pl.A.data(), (int64_t)pl.A.size(), pl.vA.data(), &H3[0]));
    if (Gb.nloc > 0) ALGP_TRY(ensure(c, c->mi.Xbar, es * (size_t)Gb.nloc * NB * mbpad));
    if (Ga.nloc > 0) ALGP_TRY(ensure(c, c->mi.Xall, es * (size_t)Ga.nloc * NB * npad));
    ALGP_TRY(mi_vectors(c, pl, mbpad + npad));
    ALGP_TRY(ensure(c, c->mi.Fold, es * npad));
    char* own = (char*)c->rowx.p;
    ALGP_HIP(hipMemsetAsync(own, 0, pl.cbytes, c->stream));
    for (int which = 0; which < 2; ++which) {
        const MiGroup& G = which ? Ga : Gb;
        if (G.member < 0 || G.m == 0) continue;
        // C_AbarAbar carries no measurement noise (agent.py:331), C + D_all every site's
        ALGP_TRY(ensure(c, c->mi.Full, es * (size_t)G.mpad * G.mpad));
        int64_t mp;
        ALGP_TRY(build_set_matrix(c, which ? pl.all.data() : pl.Abar.data(), G.m, which ? pl.vall.data() : nullptr, &mp, p(c->mi.Full)));
        double ld = 0;
        ALGP_TRY(factor_resident(c, p(c->mi.Full), G.m, G.mpad, p(c->auxInv), SC_AUXLOGDET, SC_AUXINFO, &ld));
        H3[1 + which] = (double)G.m * ENT_CONST + 0.5 * ld;
        T* X = p(which ? c->mi.Xall : c->mi.Xbar);
        ALGP_TRY(mi_trinv_rows<T>(c, {.klass = ALGP_PROF_GEMM_OTHER, .X = X, .ldx = G.mpad, .L = p(c->mi.Full), .npad = G.mpad, .ldl = G.mpad, .invD = p(c->auxInv)},
                                  G.nloc, G.g, G.member));
        T* dst = (T*)(own + 32 + (which ? es * NB * (size_t)Gb.maxloc : 0));
        if (G.nloc > 0) ALGP_TRY(rows_reduce_launch<T>(c, X, G.nloc * NB, G.mpad, G.mpad, (const T*)nullptr, dst, (T*)nullptr, 0));
    }
    ALGP_TRY(sync(c));
    release(c, c->mi.Full);                                  // this rank's rows exist: the factor goes
    return ALGP_OK;
}

// fold the next committed pick (q = mi.npicks) into the whole diagonals on every rank: two gathers, see the top of the file
template <typename T>
int Impl<T>::mi_shard_fold(algp_ctx* c, int st) {
    MiState& mi = c->mi;
    const int64_t n = c->n_pool, npad = mi.npad, mbpad = mi.mbpad, mb = mi.mb;
    const MiGroup Gb = mi_group(c, 0, mb, mbpad), Ga = mi_group(c, 1, n, npad);
    const size_t es = sizeof(T);
    size_t rbytes, cbytes;
    mi_payloads(c, mb, mbpad, npad, es, &rbytes, &cbytes);
    const int64_t q = mi.npicks;
    st = comm_fold_status(c, st, mi.holds(1), "the sharded mutual-information state", q, "mutual_information", &c->debug_fail_next_mi);
    PickRec pk;
    pk.pool_idx = 0;
    pk.in_train = 1;
    int64_t cb = -1;
    if (st == ALGP_OK) {
        pk = c->picks[(size_t)q];
        if (!pk.in_train) {
            cb = mi.posbar[pk.pool_idx];
            if (cb < 0) st = fail(c, ALGP_ERR_STATE, "mutual_information: a picked site is missing from the complement set");
        }
    }
    char* own = (char*)c->rowx.p;
    // 1. the rows of X at the pick, from the ranks that hold them
    if (st == ALGP_OK && cb >= 0 && Gb.member >= 0 && (cb / NB) % Gb.g == Gb.member) {
        const int64_t lr = cb / NB / Gb.g * NB + cb % NB;
        if (hipMemcpyAsync(own + 32, p(mi.Xbar) + lr * mbpad, es * mbpad, hipMemcpyDeviceToDevice, c->stream) != hipSuccess)
            st = fail(c, ALGP_ERR_HIP, "greedy_sharded: copying this rank's row of the complement's inverse failed");
    }
    if (st == ALGP_OK && Ga.member >= 0 && (pk.pool_idx / NB) % Ga.g == Ga.member) {
        const int64_t lr = pk.pool_idx / NB / Ga.g * NB + pk.pool_idx % NB;
        if (hipMemcpyAsync(own + 32 + es * mbpad, p(mi.Xall) + lr * npad, es * npad, hipMemcpyDeviceToDevice, c->stream) != hipSuccess)
            st = fail(c, ALGP_ERR_HIP, "greedy_sharded: copying this rank's row of the pool's inverse failed");
    }
    ALGP_TRY(comm_exchange(c, MI_STATE, "the row exchange of a pick", rbytes, st));
    // 2. this rank's entries of the pick's columns, the earlier picks' terms removed
    const char* rows = own + rbytes;
    const int r = (int)(q - mi.base);
    double* Hs = (double*)mi.H.p;
    if (cb >= 0 && Gb.nloc > 0) {
        const T* xc = (const T*)(rows + (size_t)(Gb.first + (cb / NB) % Gb.g) * rbytes + 32);
        st = rows_reduce_launch<T>(c, p(mi.Xbar), Gb.nloc * NB, mbpad, mbpad, xc, (T*)nullptr, p(mi.Col), cb / NB * NB);
        if (st == ALGP_OK)
            st = mi_cols_local_launch<T>(c, Gb.nloc * NB, Gb.g, Gb.member, mb, p(mi.Col), p(mi.U), mbpad, Hs + 3, (int)mi.nbar,
                                         cb, (T*)(own + 32));
    }
    if (st == ALGP_OK && Ga.nloc > 0) {
        const T* xc = (const T*)(rows + (size_t)(Ga.first + (pk.pool_idx / NB) % Ga.g) * rbytes + 32 + es * mbpad);
        st = rows_reduce_launch<T>(c, p(mi.Xall), Ga.nloc * NB, npad, npad, xc, (T*)nullptr, p(mi.Col) + mbpad,
                                   pk.pool_idx / NB * NB);
        if (st == ALGP_OK)
            st = mi_cols_local_launch<T>(c, Ga.nloc * NB, Ga.g, Ga.member, n, p(mi.Col) + mbpad, p(mi.W), npad,
                                         Hs + 3 + MAX_APPEND, r, pk.pool_idx, (T*)(own + 32 + es * NB * (size_t)Gb.maxloc));
    }
    ALGP_TRY(comm_exchange(c, MI_STATE, "the column exchange of a pick", cbytes, st));
    // 3. on every rank: the whole columns, folded into both diagonals (mi_rank1_kernel at the next slot of each list)
    const char* pcs = own + cbytes;
    const LazyPick* lp = (const LazyPick*)c->lazypicks.p + q;
    const double delta = 1.0 / (1.0 / mi.ss + 1.0 / mi.sm) - mi.sm;
    if (cb >= 0) {
        const int64_t nb = mi.nbar;
        ALGP_TRY(mi_assemble_launch<T>(c, mb, Gb.g, Gb.first, pcs, (int64_t)cbytes, 32, p(mi.Fold)));
        ALGP_TRY(mi_rank1_launch<T>(c, mb, p(mi.Fold), p(mi.U) + nb * mbpad, mbpad, Hs + 3 + nb, 0, cb, 0, 0.0, p(mi.DP), Hs + 1,
                                    (double*)nullptr, lp));
        mi.nbar += 1;
    }
    ALGP_TRY(mi_assemble_launch<T>(c, n, Ga.g, Ga.first, pcs, (int64_t)cbytes, (int64_t)(32 + es * NB * (size_t)Gb.maxloc), p(mi.Fold)));
    ALGP_TRY(mi_rank1_launch<T>(c, n, p(mi.Fold), p(mi.W) + (int64_t)r * npad, npad, Hs + 3 + MAX_APPEND + r, 0, pk.pool_idx, 1,
                                pk.in_train ? delta : mi.ss, p(mi.DQ), Hs + 2, Hs + 0, lp));
    mi.npicks += 1;
    return ALGP_OK;
}

// Bring the sharded MI state up to the committed picks, on every rank together.  st: this rank's status so far (it still
// takes part in every collective).  first_of_call: the first pick of an algp_greedy_sharded call -- an agreement word
// decides whether every rank (re)builds; later picks of the call fold the one pick committed since, with two gathers.
template <typename T>
int Impl<T>::mi_shard_step(algp_ctx* c, double ss, double sm, int st, bool first_of_call) {
    int64_t rounds = 1;
    if (first_of_call) {
        MiPlan pl;
        const bool need = !c->mi.current(1, ss, sm, (int64_t)c->picks.size());
        // every rank plans and checks its memory, whether or not it needs the build: any rank's need is everybody's
        if (st == ALGP_OK) st = mi_shard_plan(c, ss, sm, pl);
        if (st == ALGP_OK) st = comm_rows_reserve(c, std::max(pl.rbytes, pl.cbytes));   // the exchange's staging (MB)
        // field 1: whether this rank needs a build, and its layout (2 n_complement + need): a rank attached with another
        // split would gather other byte counts, so the layouts are compared before any payload travels
        const double mine[4] = {(double)st, 2.0 * c->mi.ncomp + (need ? 1.0 : 0.0), (double)c->picks.size(), (double)c->mi.npicks};
        std::vector<double> all;
        ALGP_TRY(comm_agree_checked(c, MI_STATE, "the plan", mine, all));
        bool any_need = false, same_layout = true;
        for (int r = 0; r < c->comm_nranks; ++r) same_layout = same_layout && ((int64_t)all[(size_t)r * 4 + 1] >> 1) == (int64_t)c->mi.ncomp;
        if (!same_layout) {
            c->mi.valid = false;
            std::string got;
            for (int r = 0; r < c->comm_nranks; ++r) got += (r ? ", " : "") + std::to_string((int64_t)all[(size_t)r * 4 + 1] >> 1);
            return fail(c, ALGP_ERR_BAD_ARG, "greedy_sharded: the ranks attached different MI layouts (n_complement_ranks per rank: " +
                                                 got + "); call algp_comm_set_mi_groups with the same value on every rank");
        }
        ALGP_TRY(comm_picks_agree(c, MI_STATE, "greedy_sharded", all, 4, 1, &any_need));
        if (any_need) {
            double H3[3] = {0.0, 0.0, 0.0};
            const int bst = mi_shard_build(c, pl, H3);
            std::vector<double> hdr;
            ALGP_TRY(comm_exchange(c, MI_STATE, "the build", pl.cbytes, bst, H3, &hdr));
            // whole diagonals from the pieces, the entropies from the first rank of each group
            const MiGroup Gb = mi_group(c, 0, pl.mb, pl.mbpad), Ga = mi_group(c, 1, c->n_pool, pl.npad);
            const char* pcs = (const char*)c->rowx.p + pl.cbytes;
            ALGP_TRY(mi_assemble_launch<T>(c, pl.mb, Gb.g, Gb.first, pcs, (int64_t)pl.cbytes, 32, p(c->mi.DP)));
            ALGP_TRY(mi_assemble_launch<T>(c, c->n_pool, Ga.g, Ga.first, pcs, (int64_t)pl.cbytes,
                                           (int64_t)(32 + sizeof(T) * NB * (size_t)Gb.maxloc), p(c->mi.DQ)));
            const double Hs[3] = {hdr[1], pl.mb > 0 ? hdr[(size_t)Gb.first * 4 + 2] : 0.0, hdr[(size_t)Ga.first * 4 + 3]};
            ALGP_TRY(mi_install(c, pl, Hs, 1, ss, sm));
        }
        rounds = (int64_t)c->picks.size() - c->mi.npicks;    // the same on every rank (agreed above)
    }
    return comm_catch_up(c, rounds, st, &Impl<T>::mi_shard_fold);
}

template struct Impl<float>;
template struct Impl<double>;

}  // namespace algp

extern "C" {

int algp_comm_set_mi_groups(algp_ctx* c, int n_complement_ranks) {
    CHECK_CTX(c);
    if (n_complement_ranks <= 0) {
        c->mi.drop_layout();
        return ALGP_OK;
    }
    if (!c->comm && !c->host_gather) return fail(c, ALGP_ERR_STATE, "comm_set_mi_groups: call algp_comm_init (or algp_comm_init_host) first");
    const int nr = c->comm_nranks;
    if (nr == 1 ? n_complement_ranks != 1 : n_complement_ranks >= nr)
        return fail(c, ALGP_ERR_BAD_ARG, "comm_set_mi_groups: 1 <= n_complement_ranks < world (a world of one: 1, the rank holds both matrices)");
    if (c->mi.ncomp != n_complement_ranks) c->mi.drop_layout();
    c->mi.ncomp = n_complement_ranks;
    return ALGP_OK;
}

}  // extern "C"
