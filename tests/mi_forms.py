"""The mutual-information criterion's utilities (agent.py:330-339) in NumPy fp64, and how the suite compares them: what
tests/test_mi_regimes.py and tests/test_mi_forms_host.py stand on.

A utility is u_i = H(A u i) + H(Abar \\ i) - H(all_i).  H(A) + H(Abar) - H(all) of the state being scored is common to
every candidate and is the whole pool's entropy (hundreds of nats); the part that decides a pick is the spread between
candidates (O(1)).  An error bound relative to max|u| is therefore a bound on the common offset only, so `compare` splits
the error e = got - want in two:

    the offset          |median e|            <= b_off (|H(A)| + |H(Abar)| + |H(all)|)
    per candidate       max|e - median e|     <= b_c max(1, max|want - median want|)

b_off: 1e-9 (fp64), 1e-4 (fp32) -- the offset is a sum of three log-determinant entropies; 1e-4 relative is the suite's fp32
bar for a log-determinant (tests/test_hip_kernels.py) and 1e-9 its fp64 greedy bar (tests/test_greedy_regimes.py: _ut_bound).
b_c: 1e-9 (fp64), 1e-3 (fp32) -- _ut_bound's bars for the O(1) entropy utilities: an MI utility with its shared offset
removed is the same kind of quantity.  With fewer than 8 live rows the mean stands in for the median.

Three pieces:
  reference  oracle.gp_oracle.greedy_fast along forced picks, with (H(A), H(Abar), H(all)) of every state scored;
  terms / utilities_from_terms   the same utilities from dense solves of the three sets, independent of greedy_fast's rank-1
             algebra, with the MUTATIONS the host test feeds to `compare` (a wrong complement row, a unit-row pick folded
             with ss in place of delta);
  cases / problem / forced_picks   the seeded problems both test files share.
"""
import functools
import types

import numpy as np

import matern_forms as MF
from oracle import gp_oracle as O

S_STD, M_STD = 0.1, 1.0
B_OFF = {np.dtype(np.float64): 1e-9, np.dtype(np.float32): 1e-4}
B_C = {np.dtype(np.float64): 1e-9, np.dtype(np.float32): 1e-3}
MEDIAN_ROWS = 8                                   # fewer live rows: the mean in place of the median
LOG_NOISE = np.log(1e-2)


def _noise(static, mobile, ss, sm):
    """Every site's measurement noise (0: not sampled)."""
    vf = 1.0 / (1.0 / ss + 1.0 / sm)
    return np.where(static & mobile, vf, np.where(static, ss, np.where(mobile, sm, 0.0)))


def entropies(C, static, mobile, ss, sm):
    """(H(A), H(Abar), H(all)) of one state, as oracle._mi_extra_terms forms them."""
    sampled = static | mobile
    A = np.where(sampled)[0]
    B = np.where(~sampled)[0]
    v = _noise(static, mobile, ss, sm)
    return (O.entropy_from_cov_chol(C[np.ix_(A, A)] + np.diag(v[A])), O.entropy_from_cov_chol(C[np.ix_(B, B)]),
            O.entropy_from_cov_chol(C + np.diag(v)))


def reference(C, static, mobile, ss_std, sm_std, forced):
    """Utilities over the pool of every pick along `forced` (oracle.greedy_fast, -inf where a site is not a live
    candidate), and (H(A), H(Abar), H(all)) of the state each pick was scored in: (ut[k, n], H[k, 3])."""
    forced = [int(f) for f in forced]
    static = np.asarray(static, bool)
    mobile = np.asarray(mobile, bool)
    _, ut = O.greedy_fast(C, static, mobile, ss_std, sm_std, len(forced), 'mutual_information', forced_picks=forced)
    cur = static.copy()
    H = []
    for f in forced:
        H.append(entropies(C, cur, mobile, ss_std ** 2, sm_std ** 2))
        cur[f] = True
    return ut, np.array(H).reshape(len(forced), 3)


def free_picks(C, static, mobile, ss_std, sm_std, k):
    """The oracle's own k picks under the criterion."""
    picks, _ = O.greedy_fast(C, static, mobile, ss_std, sm_std, k, 'mutual_information')
    return [int(q) for q in picks]


# ------------------------------------------------------------------ the comparison
def measure(got, want, unit, entropies):
    """The figures `compare` bounds, without a bound: offset and per-candidate error (over all live rows, over the unit
    rows, over the new-site rows), the spread of `want` and the sum of the entropies' magnitudes.  The rows live in
    `want` are measured; rows live in only one of the two are counted in `mask`."""
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    live = np.isfinite(want)
    m = types.SimpleNamespace(mask=int(np.sum(np.isfinite(got) != live)), rows=int(live.sum()), off=0.0, per=0.0,
                              per_unit=0.0, per_new=0.0, spread=0.0, hsum=float(np.sum(np.abs(np.asarray(entropies, np.float64)))))
    both = live & np.isfinite(got)
    if not both.any():
        return m
    centre = np.median if both.sum() >= MEDIAN_ROWS else np.mean
    e = got[both] - want[both]
    m.off = float(centre(e))
    dev = np.abs(e - m.off)
    u = np.asarray(unit, bool)[both]
    m.per = float(np.max(dev))
    m.per_unit = float(dev[u].max()) if u.any() else 0.0
    m.per_new = float(dev[~u].max()) if (~u).any() else 0.0
    m.spread = float(np.max(np.abs(want[both] - centre(want[both]))))
    return m


def compare(got, want, unit, dt, entropies, what=''):
    """Assert the two bounds of the module text on one candidate list; returns (offset error, per-candidate error).
    `unit` marks the mobile-sampled rows: the message splits the per-candidate error by kind of row."""
    m = measure(got, want, unit, entropies)
    dt = np.dtype(dt)
    assert m.mask == 0, '%s: %d rows are live in one of the two only' % (what, m.mask)
    assert abs(m.off) <= B_OFF[dt] * m.hsum, '%s: offset %.3e > %.0e x %.3f' % (what, m.off, B_OFF[dt], m.hsum)
    assert m.per <= B_C[dt] * max(1.0, m.spread), '%s: per-candidate %.3e (unit rows %.2e, new-site rows %.2e) > %.0e x max(1, %.3f)' % (
        what, m.per, m.per_unit, m.per_new, B_C[dt], m.spread)
    return abs(m.off), m.per


def centred(a, b):
    """max|(a - b) - centre(a - b)| over the rows live in both: the size of a mutation once its common offset is gone."""
    live = np.isfinite(a) & np.isfinite(b)
    if not live.any():
        return 0.0
    e = a[live] - b[live]
    return float(np.max(np.abs(e - (np.median(e) if live.sum() >= MEDIAN_ROWS else np.mean(e)))))


# ------------------------------------------------------------------ dense terms and the mutations
def terms(C, static, mobile, ss, sm, noise_all=None):
    """The pieces of every candidate's utility in one state, from dense solves of the three sets: the entropy gain of the
    train set, diag(C_AbarAbar^-1), diag((C + D_all)^-1) and the three entropies.  `noise_all` overrides the noise of the
    whole pool's matrix alone (mutation d)."""
    n = len(C)
    sampled = static | mobile
    A = np.where(sampled)[0]
    B = np.where(~sampled)[0]
    v = _noise(static, mobile, ss, sm)
    t = types.SimpleNamespace(n=n, static=static.copy(), mobile=mobile.copy(), ss=ss, sm=sm, A=A, B=B)
    t.posb = -np.ones(n, np.int64)
    t.posb[B] = np.arange(len(B))
    Sinv = np.linalg.inv(C[np.ix_(A, A)] + np.diag(v[A])) if len(A) else np.zeros((0, 0))
    t.sjj = np.zeros(n)
    t.sjj[A] = np.diag(Sinv)
    t.pv = np.diag(C) - np.einsum('ia,ab,ib->i', C[:, A], Sinv, C[:, A])
    t.invb = np.diag(np.linalg.inv(C[np.ix_(B, B)])) if len(B) else np.zeros(0)
    va = v if noise_all is None else noise_all
    t.invall = np.diag(np.linalg.inv(C + np.diag(va)))
    t.H = np.array([O.entropy_from_cov_chol(C[np.ix_(A, A)] + np.diag(v[A])), O.entropy_from_cov_chol(C[np.ix_(B, B)]),
                    O.entropy_from_cov_chol(C + np.diag(va))])
    return t


def utilities_from_terms(t, row_shift=0):
    """u over the pool (-inf at static sites).  row_shift: the complement row a new site reads, off by that many
    (mutation c)."""
    H = t.H
    delta = 1.0 / (1.0 / t.ss + 1.0 / t.sm) - t.sm
    u = np.full(t.n, -np.inf)
    unit = t.mobile & ~t.static
    new = ~t.mobile & ~t.static
    u[unit] = 0.5 * np.log1p(delta * t.sjj[unit]) + H[0] + H[1] - (H[2] + 0.5 * np.log1p(delta * t.invall[unit]))
    if new.any():
        rows = (t.posb[new] + row_shift) % len(t.B)
        u[new] = (O.CONST + 0.5 * np.log(t.pv[new] + t.ss)) + H[0] + (H[1] - O.CONST + 0.5 * np.log(t.invb[rows])) \
            - (H[2] + 0.5 * np.log1p(t.ss * t.invall[new]))
    return u


# ------------------------------------------------------------------ the problems
# kernel ids of include/algp_hip.h (matern_forms)
RBF, M15, M05, M25 = MF.RBF, MF.MATERN15, MF.MATERN05, MF.MATERN25


def _case(key, n, mb, n_static, overlap, D=2, kid=RBF, explicit=False, picks=('free', 4), check=None, seed=0, fixed=None):
    """n sites of which mb are not sampled, n_static static and `overlap` of those mobile-sampled too; the other
    n - mb - n_static are mobile-sampled only (the unit rows).  picks: how forced_picks chooses; check: the picks whose
    utilities are compared (all when None); fixed: {pool index: 'new' | 'unit'} sites whose kind is set by hand."""
    return types.SimpleNamespace(key=key, n=n, mb=mb, n_static=n_static, overlap=overlap, D=D, kid=kid, explicit=explicit,
                                 picks=picks, check=check, seed=seed, fixed=fixed or {})


_EDGE = lambda n: {0: 'new', n - 1: 'new', 127: 'unit', 128: 'unit'}


def cases():
    """Every problem of tests/test_mi_regimes.py, by key."""
    cs = [
        # set shapes
        _case('all_mobile_n130', 130, 0, 0, 0, picks=('units', 2)),
        _case('one_unsampled_n200', 200, 1, 60, 20, picks=('alternate', 4)),
        _case('empty_train_n129', 129, 129, 0, 0, picks=('free', 4)),
        _case('mb127_n260', 260, 127, 50, 15, picks=('alternate', 4)),
        _case('mb128_n260', 260, 128, 50, 15, picks=('alternate', 4)),
        _case('mb129_n260', 260, 129, 50, 15, picks=('alternate', 4)),
        _case('pool_n128', 128, 60, 25, 8, picks=('alternate', 4)),
        _case('pool_n129', 129, 60, 25, 8, picks=('alternate', 4)),
        _case('pool_n512', 512, 250, 100, 30, picks=('alternate', 4)),
        _case('pool_n513', 513, 250, 100, 30, picks=('alternate', 4)),
        _case('pool_n640', 640, 300, 120, 40, picks=('alternate', 4)),
        _case('pool_n1153', 1153, 600, 200, 60, picks=('alternate', 4)),
        # pick positions: eight picks, so that four new sites can sit at the complement rows 0, 127, 128 and mb - 1
        _case('edges_n300', 300, 160, 40, 10, picks=('edges', 8), fixed=_EDGE(300)),
        _case('edges_n650', 650, 300, 120, 40, picks=('edges', 8), fixed=_EDGE(650)),
        # full lists: 128 new sites fill both rank-1 lists; 96 new and 32 mobile-sampled sites fill the pool's with both signs
        _case('full_new_n300', 300, 180, 40, 10, picks=('new', 128), check=(0, 1, 63, 126, 127)),
        _case('full_mixed_n300', 300, 160, 40, 10, picks=('mixed', 128), check=(0, 1, 63, 126, 127)),
        # widths and forms
        _case('D1_rbf_n513', 513, 250, 100, 30, D=1, kid=RBF),
        _case('D3_matern05_n513', 513, 250, 100, 30, D=3, kid=M05, picks=('alternate', 4)),
        _case('D5_matern15_n513', 513, 250, 100, 30, D=5, kid=M15),
        _case('D8_matern25_n513', 513, 250, 100, 30, D=8, kid=M25, picks=('alternate', 4)),
        _case('D8_rbf_n513', 513, 250, 100, 30, D=8, kid=RBF, picks=('alternate', 4)),
        _case('D1_matern25_n513', 513, 250, 100, 30, D=1, kid=M25),
        _case('D3_matern15_n513', 513, 250, 100, 30, D=3, kid=M15, picks=('alternate', 4)),
        _case('explicit_cov_n513', 513, 250, 100, 30, D=2, kid=M15, explicit=True, picks=('alternate', 4)),
    ]
    for i, c in enumerate(cs):
        c.seed = 100 + i
    return {c.key: c for c in cs}


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def problem(key):
    """Coordinates uniform on a box of side 2.2 n^(1/D) (rounded to float32, so that one reference serves both precisions),
    one length-scale per dimension from [1.2, 2.0], outputscale 1, sigma_n^2 = 1e-2; C = K + sigma_n^2 I."""
    cs = cases()[key]
    rng = np.random.RandomState(cs.seed)
    n, D = cs.n, cs.D
    X = _f32(rng.uniform(0.0, 2.2 * n ** (1.0 / D), (n, D)))
    log_ls = np.log(rng.uniform(1.2, 2.0, D))
    hand = np.array(sorted(cs.fixed), np.int64)
    rest = rng.permutation(np.setdiff1d(np.arange(n), hand))
    n_new = sum(1 for v in cs.fixed.values() if v == 'new')
    n_unit = len(cs.fixed) - n_new
    static = np.zeros(n, bool)
    mobile = np.zeros(n, bool)
    a, b = cs.mb - n_new, cs.mb - n_new + cs.n_static                # rest[:a] unsampled, rest[a:b] static, rest[b:] mobile only
    static[rest[a:b]] = True
    mobile[rest[b - cs.overlap:]] = True
    for i, kind in cs.fixed.items():
        mobile[i] = kind == 'unit'
    p = types.SimpleNamespace(key=key, case=cs, n=n, D=D, X=X, kid=cs.kid, explicit=cs.explicit, log_ls=log_ls, log_os=0.0,
                              log_noise=LOG_NOISE, static=static, mobile=mobile, rng=rng)
    p.C = MF.kernel_matrix(cs.kid, log_ls, 0.0, X) + np.exp(LOG_NOISE) * np.eye(n)
    p.A = np.where(static | mobile)[0]
    p.Abar = np.where(~(static | mobile))[0]
    assert len(p.Abar) == cs.mb and int(static.sum()) == cs.n_static and len(p.A) - cs.n_static == n - cs.mb - cs.n_static
    ss, sm = S_STD ** 2, M_STD ** 2
    p.var = _noise(static, mobile, ss, sm)[p.A]
    p.cand = np.where(~static)[0]
    p.unit = mobile[p.cand]
    p.memo = {}
    return p


def forced_picks(p):
    """The case's pick sequence, found with the oracle and the sets alone.
      free       the oracle's own picks
      alternate  new site, mobile-sampled site, ...: the oracle's best of that kind in the state reached so far
      new / units   sites of one kind in a seeded order
      mixed      three new sites, one mobile-sampled site, ... in a seeded order.  The states checked in a list of 128 (before
                 picks 2, 64, 127, 128) then follow a new site's fold: late in a long list the fold of a mobile-sampled site
                 moves the centred utilities by less than the fp32 per-candidate bar (6e-4 measured with the oracle when
                 pick 126 was one), so a dropped fold of that kind could not be told from rounding there
      edges      new sites at the complement rows 0, 127, 128 and mb - 1 (pool sites 0 and n - 1 among them), between them the
                 mobile-sampled pool sites 127 and 128 and two more."""
    if 'forced' in p.memo:
        return p.memo['forced']
    kind, k = p.case.picks
    new = np.where(~p.static & ~p.mobile)[0]
    units = np.where(~p.static & p.mobile)[0]
    order = np.random.RandomState(p.case.seed + 7)
    if kind == 'free':
        out = free_picks(p.C, p.static, p.mobile, S_STD, M_STD, k)
    elif kind == 'new':
        out = [int(q) for q in order.permutation(new)[:k]]
    elif kind == 'units':
        out = [int(q) for q in order.permutation(units)[:k]]
    elif kind == 'edges':
        assert k == 8 and p.Abar[0] == 0 and p.Abar[-1] == p.n - 1 and p.mobile[127] and p.mobile[128] and len(p.Abar) > 130
        other = [int(q) for q in order.permutation(np.setdiff1d(units, [127, 128]))[:2]]
        out = [0, 127, int(p.Abar[127]), 128, int(p.Abar[128]), other[0], p.n - 1, other[1]]
    elif kind == 'mixed':
        a, b = list(order.permutation(new)), list(order.permutation(units))
        out = [int((b if q % 4 == 3 else a).pop()) for q in range(k)]
    else:
        assert kind == 'alternate'
        out = []
        cur = p.static.copy()
        for q in range(k):
            ut = O.greedy_fast(p.C, cur, p.mobile, S_STD, M_STD, 1, 'mutual_information')[1][0]
            pool = new if (q % 2 == 0 and len(np.setdiff1d(new, out))) else units
            pool = np.setdiff1d(pool, out)
            out.append(int(pool[int(np.argmax(ut[pool]))]))
            cur[out[-1]] = True
    assert len(set(out)) == len(out) == k and not p.static[out].any()
    p.memo['forced'] = out
    return out


def case_reference(p):
    """reference() along the case's forced picks, once per problem."""
    if 'ref' not in p.memo:
        p.memo['ref'] = reference(p.C, p.static, p.mobile, S_STD, M_STD, forced_picks(p))
        for a in p.memo['ref']:
            a.setflags(write=False)
    return p.memo['ref']
