"""tests/path_forms.py on the host: its helpers against the oracle and against the closed form of tests/test_paths_vr_host.py, and
the conditions that the per-path bounds of tests/test_path_regimes.py rest on -- cond(S_A) and cond of every path's block at most
1e3, the route every case must take, the path count that makes the variance-reduction scorer run a second batch, and the margins
(finite references, no utility a bound divides by below 1e-6, the top two utilities apart where the argmax is asserted).

Nothing here needs a device.
"""
import os
import re
import types

import numpy as np
import pytest

import matern_forms as MF
import path_forms as PF
import test_paths_vr_host as VH
from oracle import gp_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE_KERNELS = [pytest.param(name, kid, id='%s-%s' % (name, PF.KNAMES[kid])) for name in PF.CASES for kid in PF.kernels_of(name)]
SMALL_CASES = ['shape_maxlen5', 'rm_row0_rowN_lds', 'len63', 'shape_maxlen70_64distinct']


def _close(a, b, tol):
    return abs(a - b) <= tol * max(1.0, abs(b))


@pytest.mark.parametrize('kid', PF.KERNELS_EVERYWHERE, ids=['rbf', 'matern15'])
def test_entropy_and_mi_helpers_equal_the_oracle(kid):
    """O.best_path_ref scores the fused form: one row per site, a re-measured site's noise v sm / (v + sm).  The entropy helper
    counts a second row instead, which differs by CONST + 1/2 log(v + sm) per re-measured site (include/algp_hip.h)."""
    assert PF.CONST == O.CONST
    p = PF.problem('small', kid)
    hyp = O.Hypers(p.log_ls, p.log_os, p.log_noise, kid)
    assert np.max(np.abs(O.kernel_matrix(hyp, p.X) + p.noise * np.eye(p.n) - p.C)) < 1e-13
    for name in SMALL_CASES:
        _, rows = PF.sites_of(name)
        lists = [PF.distinct(r) for r in rows]
        for crit in ('entropy', 'mutual_information'):
            _, ut = O.best_path_ref(p.C, p.static, p.mobile, [[]] + lists, [], PF.STATIC_STD, PF.MOBILE_STD, crit)
            for r, want in zip(rows, ut[1:] - ut[0]):
                if crit == 'entropy':
                    got = PF.entropy_gain(p, r) - PF.fuse_constant(p, r)
                else:
                    t = PF.mi_terms(p, r)
                    got = t[0] + t[1] - t[2]
                    assert _close(t[0], PF.entropy_gain(p, r) - PF.fuse_constant(p, r), 1e-10), (name, r)
                print('%s %s %-18s helper %.12e oracle %.12e' % (name, PF.KNAMES[kid], crit, got, want))
                assert _close(got, want, 1e-10), (name, crit, got, want)


@pytest.mark.parametrize('kid', PF.KERNELS_EVERYWHERE, ids=['rbf', 'matern15'])
def test_variance_reduction_helper_equals_the_closed_form(kid):
    """one refit per path against tr((Gamma_SS + sm I)^-1 Phi_SS) of tests/test_paths_vr_host.py, relative to the utility itself"""
    p = PF.problem('small', kid)
    q = types.SimpleNamespace(A=p.A, noise=p.var, free=p.free, cov=lambda r, c: p.C[np.ix_(np.asarray(r, int), np.asarray(c, int))],
                              hyp=types.SimpleNamespace(outputscale=1.0, noise=p.noise))
    for name in SMALL_CASES:
        sites, rows = PF.sites_of(name)
        closed, _ = VH.closed_form(q, sites, sm=PF.SM)
        for r, want in zip(rows, closed):
            got = PF.variance_reduction(p, r)
            print('%s %s helper %.12e closed form %.12e rel %.2e' % (name, PF.KNAMES[kid], got, want, abs(got - want) / max(abs(want), 1e-300)))
            assert abs(got - want) <= 1e-10 * abs(want), (name, got, want)


def test_weighted_helper_is_linear_in_the_weights():
    """weights w and 2 w + indicator: the weighted refit is the weighted sum of per-target reductions"""
    p = PF.problem('small', MF.RBF)
    _, rows = PF.sites_of('shape_maxlen5')
    rng = np.random.RandomState(0)
    w = PF.f32(rng.uniform(0, 2, p.n))
    one = np.ones(p.n)
    for r in rows:
        a, b, c = PF.variance_reduction(p, r, weights=w), PF.variance_reduction(p, r), PF.variance_reduction(p, r, weights=2 * w + one)
        assert abs(c - (2 * a + b)) <= 1e-10 * max(abs(c), 1e-300) or (a == b == c == 0.0)


# ---- the conditions of the bounds -------------------------------------------------------------------------------------------
def _cond(M):
    ev = np.linalg.eigvalsh(M)
    assert ev[0] > 0
    return ev[-1] / ev[0]


@pytest.mark.parametrize('name', ['small', 'mid', 'wide', 'full'])
def test_train_matrices_are_well_conditioned(name):
    kids = sorted({k for cn, c in PF.CASES.items() if c.problem.startswith(name) for k in PF.kernels_of(cn)})
    for kid in kids:
        cond = _cond(PF.problem(name, kid).SA)
        print('%s %s cond(S_A) %.1f' % (name, PF.KNAMES[kid], cond))
        assert cond <= 1e3


@pytest.mark.parametrize('name,kid', CASE_KERNELS)
def test_every_path_block_is_well_conditioned_and_every_reference_usable(name, kid):
    case = PF.CASES[name]
    p = PF.problem(case.problem, kid)
    _, rows = PF.sites_of(name)
    worst = max([_cond(PF.path_block(p, r)) for r in rows if PF.distinct(r)])
    print('%s %s worst cond of a path block %.1f' % (name, PF.KNAMES[kid], worst))
    assert worst <= 1e3
    ref = PF.reference(name, kid)
    empty = np.array([not PF.distinct(r) for r in rows])
    for what, v in ref.items():
        assert np.all(np.isfinite(v)), what
        assert np.all(v[empty] == 0.0), what                                 # exactly 0: the GPU file asserts the same bits
    if 'vr' in ref and len(p.free):
        assert np.all(ref['vr'][~empty] >= 1e-6), np.min(ref['vr'][~empty])  # the bound divides by it
    if case.argmax and len(rows) > 1:
        counts = (481, len(rows)) if name == 'vr_batches' else (len(rows),)  # fp64 scores the first 481 paths of that case
        for cnt in counts:
            for what, v in ref.items():
                if what == 'mi' and not len(p.free):
                    continue                                                 # every site sampled: H(A) = H(all), the MI is 0
                u = v[:cnt] if v.ndim == 1 else (v[:cnt, 0] + v[:cnt, 1] - v[:cnt, 2])
                top = np.sort(u)[-2:]
                assert (top[1] - top[0]) > 1e-7 * abs(top[1]), (what, top)


def test_routes_follow_from_the_lengths():
    for name, case in PF.CASES.items():
        _, rows = PF.sites_of(name)
        used = [len(PF.distinct(r)) for r in rows]
        assert max(used) <= 256
        for entry in ('ent', 'mi'):
            if entry in case.entries:
                assert case.routes[entry] == PF.route(max(used)), (name, entry)
        if 'vr' in case.entries:
            big = [k for k in used if k > 64]
            want = [PF.route(k) if k <= 64 else PF.route(max(big)) for k in used]
            assert list(case.routes['vr']) == want, name
    # the lengths at the route edges, each a call of its own, and the shapes of the site array
    for k in (1, 2, 63, 64, 65, 127, 128, 129, 255, 256):
        sites, rows = PF.sites_of('len%d' % k)
        assert all(len(PF.distinct(r)) == k for r in rows)
    shape = {n: PF.sites_of(n)[0].shape[1] for n in PF.CASES}
    assert shape['shape_maxlen5'] == 5 and shape['shape_maxlen64'] == 64 and shape['shape_maxlen70_64distinct'] == 70
    assert shape['shape_maxlen262_130sites'] == 262
    s70, r70 = PF.sites_of('shape_maxlen70_64distinct')
    assert len(PF.distinct(r70[0])) == 64 and np.sum(s70[0] >= 0) > 64
    assert PF.sites_of('shape_maxlen5')[0][1, 0] == -1 and len(PF.distinct(PF.sites_of('shape_maxlen262_130sites')[1][0])) == 130


def test_second_readings_are_where_the_cases_say():
    for name in ('rm_row0_rowN_lds', 'rm_row0_rowN_batched'):
        p = PF.problem(PF.CASES[name].problem, MF.RBF)
        _, rows = PF.sites_of(name)
        assert [sorted(p.row[s] for s in r if p.row[s] >= 0) for r in rows] == [[0], [p.N - 1], [0], [p.N - 1], [0, p.N - 1]]
    p = PF.problem('mid', MF.RBF)
    for name in ('rm_only_3_64', 'rm_only_65_3', 'rm_only_130_64'):
        assert all(p.row[s] >= 0 and p.static[s] for r in PF.sites_of(name)[1] for s in r)
    r = PF.sites_of('rm_at_127_128_129')[1][0]
    assert [i for i, s in enumerate(r) if p.row[s] >= 0] == [127, 128, 129] and len(PF.distinct(r)) == 200
    p = PF.problem('wide', MF.RBF)
    assert p.N == 2100 and (p.N + 127) // 128 * 128 > 2048
    tr = {n: sorted(int(p.row[s]) for s in PF.sites_of(n)[1][0] if p.row[s] >= 0) for n in PF.CASES if n.startswith('wide')}
    assert len(tr['wide_3_row2090']) == 1 and tr['wide_3_row2090'][0] >= 2090
    assert tr['wide_65_rows5_2090'][0] == 5 and tr['wide_65_rows5_2090'][1] >= 2090 and len(tr['wide_65_rows5_2090']) == 2
    assert len(tr['wide_130_forty_rows_2048']) == 40 and tr['wide_130_forty_rows_2048'][0] >= 2048
    p = PF.problem('full', MF.RBF)
    assert p.N == p.n == 40 and not len(p.free) and len(p.st) == 40
    p = PF.problem('small', MF.RBF)
    assert p.N == 129 and len(p.st) >= 70
    p = PF.problem('mid', MF.RBF)
    assert p.N == 300 and len(p.st) >= 260 and p.D == 5
    assert len(PF.problem('mid400', MF.RBF).cand) == 400


def test_the_batching_case_runs_a_second_batch():
    """These numbers mirror api_paths_vr.hip: bmax = min(nbig, 1e9 / (4 ppad^2 sizeof(T)), 65535) paths per batch at ppad = 256.
    A change there turns this test red instead of silently un-covering the p0 += bmax loop."""
    text = open(os.path.join(REPO, 'algp_amd', 'csrc', 'api_paths_vr.hip')).read()
    m = re.search(r'const int bmax = \(int\)std::max<int64_t>\(1, std::min<int64_t>\(\{\(int64_t\)nbig_max, \(int64_t\)(\w+) / '
                  r'\(int64_t\)\((\d+) \* mat_max \* sizeof\(T\)\), (\d+)\}\)\);', text)
    assert m, 'the batch size of score_paths_vr is not where this test reads it'
    budget, mats, cap = float(m.group(1)), int(m.group(2)), int(m.group(3))
    assert re.search(r'const size_t mat_max = \(size_t\)ppad_max \* ppad_max;', text)
    assert re.search(r'if \(used\[pth\] > NB\) ppad_max = 2 \* NB;', text)
    _, rows = PF.sites_of('vr_batches')
    used = [len(PF.distinct(r)) for r in rows]
    assert used[0] == 129 and set(used[1:]) == {65} and len(rows) == 961
    for size, count in ((8, 481), (4, 961)):
        bmax = min(count, int(budget) // (mats * 256 * 256 * size), cap)
        print('sizeof(T) = %d: %d paths per batch, %d paths' % (size, bmax, count))
        assert bmax < count <= 2 * bmax                                      # two batches, the second a partial one
        assert mats * 256 * 256 * size * bmax <= 1.01e9                      # about 1 GB of the library's scratch
