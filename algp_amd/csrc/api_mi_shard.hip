// api_mi_shard.hip -- the MI criterion's pool-wide inverses dealt over the ranks of a communicator (algp_comm_set_mi_groups),
// so that algp_greedy_sharded scores the MI criterion too.
//
// One GPU (api_greedy.hip: mi_build / mi_apply_pick) keeps X = L^-T for P = C_AbarAbar^-1 and for Q = (C + D_all)^-1 and
// reads three things from them: diag(P)_i = |X_i,:|^2, a committed pick's column P_:,c = X X_c,:^T, and the rank-1 folds of
// mi_rank1_kernel (which need only that column and the earlier picks' columns).  Whoever holds a set of ROWS of X can
// therefore compute those rows' diagonal entries and their entries of every later column; the only input from outside is
// row c itself.  Here ranks [0, g_bar) hold the complement matrix and ranks [g_bar, world) the whole pool's (a world of one
// never comes here: greedy_picks keeps the one-GPU state, mi_build, for it).  Inside a group every member builds and factors the group's matrix (replicated, no communication),
// computes only its own 128-row blocks of X (blocks member, member + g, ...: mi_trinv_rows, mi_shard.hip) and releases the
// factor.  The diagonals, the rank-1 lists U / W, their signs and the three entropies stay WHOLE on every rank, so scoring is
// mi_score_launch on each rank's own candidates.  Collectives, all of them all-gathers through comm_agree / comm_rows_gather
// (RCCL or the caller's host transport):
//   first pick of an algp_greedy_sharded call: a 32-byte agreement word (status, whether a build is needed, picks so far);
//     then, when any rank needs it, the build and ONE gather of every rank's diagonal pieces and entropies;
//   every pick folded: a gather of the owners' rows at the pick ([header | row of X_bar | row of X_all] per rank), then a
//     gather of every rank's entries of the pick's columns with the earlier terms removed; every rank puts the whole columns
//     together and folds them into its copy of both diagonals (mi_rank1_kernel, as on one GPU).
// Every gather carries each rank's status word in its 32-byte header: a rank that fails (memory, a factor that is not
// positive definite, a HIP error, an injected failure) still takes part in every collective of the step, and every rank
// returns the first failing rank's code from the same call.
#include "api_impl.h"

using namespace algp;

namespace algp {

namespace {
// one matrix's group: ranks [first, first + g), this rank's place in it (member, -1: not in it), its row tiles
struct MiGroup {
    int first = 0, g = 1, member = -1;
    int64_t m = 0, mpad = 0, nloc = 0, maxloc = 0;    // nloc: this rank's 128-row tiles; maxloc: member 0's (the most)
};
}  // namespace

// which = 0: the complement matrix (m = its sites), 1: the whole pool's; a world of at least two, 1 <= mi_ncomp < world
static MiGroup mi_group(const algp_ctx* c, int which, int64_t m, int64_t mpad) {
    MiGroup G;
    G.first = which == 0 ? 0 : c->mi_ncomp;
    G.g = which == 0 ? c->mi_ncomp : c->comm_nranks - c->mi_ncomp;
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

// this rank's header (status, three values) in front of its payload at rowx, the all-gather of `bytes` per rank, every header
// back to the host (hdr: 4 doubles per rank); code / bad: the first non-zero status in rank order and its rank (0 / -1: none)
static int mi_exchange(algp_ctx* c, size_t bytes, int st, const double* v3, std::vector<double>& hdr, int& code, int& bad) {
    const int nr = c->comm_nranks;
    c->mi_hdr[0] = (double)st;
    for (int i = 0; i < 3; ++i) c->mi_hdr[1 + i] = v3 ? v3[i] : 0.0;
    char* own = (char*)c->rowx.p;
    ALGP_HIP(hipMemcpyAsync(own, c->mi_hdr, 32, hipMemcpyHostToDevice, c->stream));
    ALGP_TRY(comm_rows_gather(c, bytes));
    hdr.assign((size_t)nr * 4, 0.0);
    ALGP_HIP(hipMemcpy2DAsync(hdr.data(), 32, own + bytes, bytes, 32, (size_t)nr, hipMemcpyDeviceToHost, c->stream));
    ALGP_TRY(sync(c));
    code = 0;
    bad = -1;
    for (int r = 0; r < nr && bad < 0; ++r)
        if (hdr[(size_t)r * 4] != 0.0) {
            bad = r;
            code = hdr[(size_t)r * 4] == hdr[(size_t)r * 4] ? (int)hdr[(size_t)r * 4] : ALGP_ERR_HIP;
        }
    return ALGP_OK;
}

// an agreed failure: the failing rank keeps its own message, the others name it; the state is rebuilt by the next call
static int mi_agreed_fail(algp_ctx* c, int code, int bad, const std::string& local_err, const char* what) {
    c->mi_valid = false;
    if (bad == c->comm_rank && !local_err.empty()) return fail(c, code, local_err);
    return fail(c, code, "greedy_sharded: rank " + std::to_string(bad) + " failed with error " + std::to_string(code) + " in " + what +
                             " of the mutual-information state; every rank returns it");
}

template <typename T>
struct Impl<T>::MiPlan {
    std::vector<int64_t> A, Abar, all, posbar;
    std::vector<T> vA, vall;
    int64_t mb = 0, mbpad = 0, npad = 0;
    size_t rbytes = 0, cbytes = 0;
};

// host side of a build: the sets (as mi_build), the sizes, and this rank's memory check -- nothing allocated yet
template <typename T>
int Impl<T>::mi_shard_plan(algp_ctx* c, double ss, double sm, MiPlan& pl) {
    const int64_t n = c->n_pool;
    if (!c->solved) return fail(c, ALGP_ERR_STATE, "greedy: call algp_solve_candidates first");
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
    const size_t held = c->auxInv.cap + c->miXbar.cap + c->miXall.cap + c->miFull.cap + c->miU.cap + c->miW.cap + c->rowx.cap;
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
    c->mi_valid = false;
    c->mi_form = 1;
    ALGP_TRY(sync(c));
    release(c, c->miXbar);                                   // whole inverses of a one-GPU build, or another layout's rows
    release(c, c->miXall);
    ALGP_TRY(set_entropy(c, pl.A.data(), (int64_t)pl.A.size(), pl.vA.data(), &H3[0]));
    if (Gb.nloc > 0) ALGP_TRY(ensure(c, c->miXbar, es * (size_t)Gb.nloc * NB * mbpad));
    if (Ga.nloc > 0) ALGP_TRY(ensure(c, c->miXall, es * (size_t)Ga.nloc * NB * npad));
    ALGP_TRY(ensure(c, c->miDP, es * mbpad));
    ALGP_TRY(ensure(c, c->miDQ, es * npad));
    ALGP_TRY(ensure(c, c->miU, es * (size_t)MAX_APPEND * mbpad));
    ALGP_TRY(ensure(c, c->miW, es * (size_t)MAX_APPEND * npad));
    ALGP_TRY(ensure(c, c->miCol, es * (size_t)(mbpad + npad)));
    ALGP_TRY(ensure(c, c->miFold, es * npad));
    ALGP_TRY(ensure(c, c->miPos, sizeof(int64_t) * n));
    ALGP_TRY(ensure(c, c->miH, sizeof(double) * (3 + 2 * MAX_APPEND)));
    char* own = (char*)c->rowx.p;
    ALGP_HIP(hipMemsetAsync(own, 0, pl.cbytes, c->stream));
    for (int which = 0; which < 2; ++which) {
        const MiGroup& G = which ? Ga : Gb;
        if (G.member < 0 || G.m == 0) continue;
        // C_AbarAbar carries no measurement noise (agent.py:331), C + D_all every site's
        ALGP_TRY(ensure(c, c->miFull, es * (size_t)G.mpad * G.mpad));
        int64_t mp;
        ALGP_TRY(build_set_matrix(c, which ? pl.all.data() : pl.Abar.data(), G.m, which ? pl.vall.data() : nullptr, &mp, p(c->miFull)));
        double ld = 0;
        ALGP_TRY(factor_resident(c, p(c->miFull), G.m, G.mpad, p(c->auxInv), SC_AUXLOGDET, SC_AUXINFO, &ld));
        H3[1 + which] = (double)G.m * ENT_CONST + 0.5 * ld;
        T* X = p(which ? c->miXall : c->miXbar);
        ALGP_TRY(mi_trinv_rows<T>(c, ALGP_PROF_GEMM_OTHER, X, G.mpad, G.nloc, G.g, G.member, p(c->miFull), G.mpad, G.mpad, p(c->auxInv)));
        T* dst = (T*)(own + 32 + (which ? es * NB * (size_t)Gb.maxloc : 0));
        if (G.nloc > 0) ALGP_TRY(rows_reduce_launch<T>(c, X, G.nloc * NB, G.mpad, G.mpad, (const T*)nullptr, dst, (T*)nullptr, 0));
    }
    ALGP_TRY(sync(c));
    release(c, c->miFull);                                   // this rank's rows exist: the factor goes
    return ALGP_OK;
}

// fold the next committed pick (q = mi_npicks) into the whole diagonals on every rank: two gathers, see the top of the file
template <typename T>
int Impl<T>::mi_shard_fold(algp_ctx* c, int st) {
    const int64_t n = c->n_pool, npad = c->mi_npad, mbpad = c->mi_mbpad, mb = c->mi_mb;
    const MiGroup Gb = mi_group(c, 0, mb, mbpad), Ga = mi_group(c, 1, n, npad);
    const size_t es = sizeof(T);
    size_t rbytes, cbytes;
    mi_payloads(c, mb, mbpad, npad, es, &rbytes, &cbytes);
    const int64_t q = c->mi_npicks;
    if (st == ALGP_OK && !(c->mi_valid && c->mi_form == 1))
        st = fail(c, ALGP_ERR_STATE, "greedy_sharded: the sharded mutual-information state is not built");
    if (st == ALGP_OK && q >= (int64_t)c->picks.size())
        st = fail(c, ALGP_ERR_STATE, "greedy_sharded: this rank has no committed pick left to fold");
    if (st == ALGP_OK && c->debug_fail_next_mi) {
        st = fail(c, c->debug_fail_next_mi, "mutual_information: failure injected by algp_debug_fail_at in the fold of a pick");
        c->debug_fail_next_mi = 0;
    }
    PickRec pk;
    pk.pool_idx = 0;
    pk.in_train = 1;
    int64_t cb = -1;
    if (st == ALGP_OK) {
        pk = c->picks[(size_t)q];
        if (!pk.in_train) {
            cb = c->mi_posbar[pk.pool_idx];
            if (cb < 0) st = fail(c, ALGP_ERR_STATE, "mutual_information: a picked site is missing from the complement set");
        }
    }
    char* own = (char*)c->rowx.p;
    // 1. the rows of X at the pick, from the ranks that hold them
    if (st == ALGP_OK && cb >= 0 && Gb.member >= 0 && (cb / NB) % Gb.g == Gb.member) {
        const int64_t lr = cb / NB / Gb.g * NB + cb % NB;
        if (hipMemcpyAsync(own + 32, p(c->miXbar) + lr * mbpad, es * mbpad, hipMemcpyDeviceToDevice, c->stream) != hipSuccess)
            st = fail(c, ALGP_ERR_HIP, "greedy_sharded: copying this rank's row of the complement's inverse failed");
    }
    if (st == ALGP_OK && Ga.member >= 0 && (pk.pool_idx / NB) % Ga.g == Ga.member) {
        const int64_t lr = pk.pool_idx / NB / Ga.g * NB + pk.pool_idx % NB;
        if (hipMemcpyAsync(own + 32 + es * mbpad, p(c->miXall) + lr * npad, es * npad, hipMemcpyDeviceToDevice, c->stream) != hipSuccess)
            st = fail(c, ALGP_ERR_HIP, "greedy_sharded: copying this rank's row of the pool's inverse failed");
    }
    std::string local_err = st != ALGP_OK ? c->err : std::string();
    std::vector<double> hdr;
    int code = 0, bad = -1;
    ALGP_TRY(mi_exchange(c, rbytes, st, nullptr, hdr, code, bad));
    if (code) return mi_agreed_fail(c, code, bad, local_err, "the row exchange of a pick");
    // 2. this rank's entries of the pick's columns, the earlier picks' terms removed
    const char* rows = own + rbytes;
    const int r = (int)(q - c->mi_base);
    double* Hs = (double*)c->miH.p;
    if (cb >= 0 && Gb.nloc > 0) {
        const T* xc = (const T*)(rows + (size_t)(Gb.first + (cb / NB) % Gb.g) * rbytes + 32);
        st = rows_reduce_launch<T>(c, p(c->miXbar), Gb.nloc * NB, mbpad, mbpad, xc, (T*)nullptr, p(c->miCol), cb / NB * NB);
        if (st == ALGP_OK)
            st = mi_cols_local_launch<T>(c, Gb.nloc * NB, Gb.g, Gb.member, mb, p(c->miCol), p(c->miU), mbpad, Hs + 3, (int)c->mi_nbar,
                                         cb, (T*)(own + 32));
    }
    if (st == ALGP_OK && Ga.nloc > 0) {
        const T* xc = (const T*)(rows + (size_t)(Ga.first + (pk.pool_idx / NB) % Ga.g) * rbytes + 32 + es * mbpad);
        st = rows_reduce_launch<T>(c, p(c->miXall), Ga.nloc * NB, npad, npad, xc, (T*)nullptr, p(c->miCol) + mbpad,
                                   pk.pool_idx / NB * NB);
        if (st == ALGP_OK)
            st = mi_cols_local_launch<T>(c, Ga.nloc * NB, Ga.g, Ga.member, n, p(c->miCol) + mbpad, p(c->miW), npad,
                                         Hs + 3 + MAX_APPEND, r, pk.pool_idx, (T*)(own + 32 + es * NB * (size_t)Gb.maxloc));
    }
    local_err = st != ALGP_OK ? c->err : std::string();
    ALGP_TRY(mi_exchange(c, cbytes, st, nullptr, hdr, code, bad));
    if (code) return mi_agreed_fail(c, code, bad, local_err, "the column exchange of a pick");
    // 3. on every rank: the whole columns, folded into both diagonals (mi_rank1_kernel at the next slot of each list)
    const char* pcs = own + cbytes;
    const LazyPick* lp = (const LazyPick*)c->lazypicks.p + q;
    const double delta = 1.0 / (1.0 / c->mi_ss + 1.0 / c->mi_sm) - c->mi_sm;
    if (cb >= 0) {
        const int64_t nb = c->mi_nbar;
        ALGP_TRY(mi_assemble_launch<T>(c, mb, Gb.g, Gb.first, pcs, (int64_t)cbytes, 32, p(c->miFold)));
        ALGP_TRY(mi_rank1_launch<T>(c, mb, p(c->miFold), p(c->miU) + nb * mbpad, mbpad, Hs + 3 + nb, 0, cb, 0, 0.0, p(c->miDP), Hs + 1,
                                    (double*)nullptr, lp));
        c->mi_nbar += 1;
    }
    ALGP_TRY(mi_assemble_launch<T>(c, n, Ga.g, Ga.first, pcs, (int64_t)cbytes, (int64_t)(32 + es * NB * (size_t)Gb.maxloc), p(c->miFold)));
    ALGP_TRY(mi_rank1_launch<T>(c, n, p(c->miFold), p(c->miW) + (int64_t)r * npad, npad, Hs + 3 + MAX_APPEND + r, 0, pk.pool_idx, 1,
                                pk.in_train ? delta : c->mi_ss, p(c->miDQ), Hs + 2, Hs + 0, lp));
    c->mi_npicks += 1;
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
        const bool need = !(c->mi_valid && c->mi_form == 1 && c->mi_ss == ss && c->mi_sm == sm &&
                            (int64_t)c->picks.size() >= c->mi_npicks);
        // every rank plans and checks its memory, whether or not it needs the build: any rank's need is everybody's
        if (st == ALGP_OK) st = mi_shard_plan(c, ss, sm, pl);
        if (st == ALGP_OK) st = comm_rows_reserve(c, std::max(pl.rbytes, pl.cbytes));   // the exchange's staging (MB)
        const std::string local_err = st != ALGP_OK ? c->err : std::string();
        // field 1: whether this rank needs a build, and its layout (2 n_complement + need): a rank attached with another
        // split would gather other byte counts, so the layouts are compared before any payload travels
        const double mine[4] = {(double)st, 2.0 * c->mi_ncomp + (need ? 1.0 : 0.0), (double)c->picks.size(), (double)c->mi_npicks};
        std::vector<double> all;
        ALGP_TRY(comm_agree(c, mine, all));
        int code = 0, bad = -1;
        bool any_need = false, same = true, same_layout = true;
        for (int r = 0; r < c->comm_nranks; ++r) {
            const double s = all[(size_t)r * 4];
            if (s != 0.0 && bad < 0) { bad = r; code = s == s ? (int)s : ALGP_ERR_HIP; }
            const int64_t f = (int64_t)all[(size_t)r * 4 + 1];
            any_need = any_need || (f & 1) != 0;
            same_layout = same_layout && (f >> 1) == (int64_t)c->mi_ncomp;
        }
        for (int r = 0; r < c->comm_nranks; ++r)    // picks so far, and (without a build) picks folded so far: equal everywhere
            same = same && all[(size_t)r * 4 + 2] == all[2] && (any_need || all[(size_t)r * 4 + 3] == all[3]);
        if (code) return mi_agreed_fail(c, code, bad, local_err, "the plan");
        if (!same_layout) {
            c->mi_valid = false;
            std::string got;
            for (int r = 0; r < c->comm_nranks; ++r) got += (r ? ", " : "") + std::to_string((int64_t)all[(size_t)r * 4 + 1] >> 1);
            return fail(c, ALGP_ERR_BAD_ARG, "greedy_sharded: the ranks attached different MI layouts (n_complement_ranks per rank: " +
                                                 got + "); call algp_comm_set_mi_groups with the same value on every rank");
        }
        if (!same) {
            c->mi_valid = false;
            return fail(c, ALGP_ERR_STATE, "greedy_sharded: the ranks hold different numbers of committed picks (a commit failed on "
                                           "one of them); re-solve the candidates on every rank");
        }
        if (any_need) {
            double H3[3] = {0.0, 0.0, 0.0};
            int bst = mi_shard_build(c, pl, H3);
            const std::string berr = bst != ALGP_OK ? c->err : std::string();
            std::vector<double> hdr;
            ALGP_TRY(mi_exchange(c, pl.cbytes, bst, H3, hdr, code, bad));
            if (code) return mi_agreed_fail(c, code, bad, berr, "the build");
            // whole diagonals from the pieces, the entropies from the first rank of each group
            const MiGroup Gb = mi_group(c, 0, pl.mb, pl.mbpad), Ga = mi_group(c, 1, c->n_pool, pl.npad);
            const char* pcs = (const char*)c->rowx.p + pl.cbytes;
            ALGP_TRY(mi_assemble_launch<T>(c, pl.mb, Gb.g, Gb.first, pcs, (int64_t)pl.cbytes, 32, p(c->miDP)));
            ALGP_TRY(mi_assemble_launch<T>(c, c->n_pool, Ga.g, Ga.first, pcs, (int64_t)pl.cbytes,
                                           (int64_t)(32 + sizeof(T) * NB * (size_t)Gb.maxloc), p(c->miDQ)));
            const double Hs[3] = {hdr[1], pl.mb > 0 ? hdr[(size_t)Gb.first * 4 + 2] : 0.0, hdr[(size_t)Ga.first * 4 + 3]};
            c->mi_posbar = pl.posbar;
            ALGP_HIP(hipMemcpyAsync(c->miH.p, Hs, sizeof(Hs), hipMemcpyHostToDevice, c->stream));
            ALGP_HIP(hipMemcpyAsync(c->miPos.p, c->mi_posbar.data(), sizeof(int64_t) * c->n_pool, hipMemcpyHostToDevice, c->stream));
            ALGP_TRY(sync(c));
            c->mi_mb = pl.mb;
            c->mi_mbpad = pl.mbpad;
            c->mi_npad = pl.npad;
            c->mi_npicks = (int64_t)c->picks.size();
            c->mi_base = c->mi_npicks;
            c->mi_nbar = 0;
            c->mi_ss = ss;
            c->mi_sm = sm;
            c->mi_valid = true;
        }
        rounds = (int64_t)c->picks.size() - c->mi_npicks;    // the same on every rank (agreed above)
    }
    for (int64_t i = 0; i < rounds; ++i) ALGP_TRY(mi_shard_fold(c, i == 0 ? st : ALGP_OK));
    return ALGP_OK;
}

template struct Impl<float>;
template struct Impl<double>;

}  // namespace algp

extern "C" {

int algp_comm_set_mi_groups(algp_ctx* c, int n_complement_ranks) {
    CHECK_CTX(c);
    if (n_complement_ranks <= 0) {
        if (c->mi_form == 1) c->mi_valid = false;
        c->mi_ncomp = 0;
        return ALGP_OK;
    }
    if (!c->comm && !c->host_gather) return fail(c, ALGP_ERR_STATE, "comm_set_mi_groups: call algp_comm_init (or algp_comm_init_host) first");
    const int nr = c->comm_nranks;
    if (nr == 1 ? n_complement_ranks != 1 : n_complement_ranks >= nr)
        return fail(c, ALGP_ERR_BAD_ARG, "comm_set_mi_groups: 1 <= n_complement_ranks < world (a world of one: 1, the rank holds both matrices)");
    if (c->mi_ncomp != n_complement_ranks && c->mi_form == 1) c->mi_valid = false;
    c->mi_ncomp = n_complement_ranks;
    return ALGP_OK;
}

}  // extern "C"
