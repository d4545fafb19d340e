"""tests/incremental_forms.py on the host (no GPU): the helper against the oracle where the two overlap, and the scripted
sequences of tests/test_incremental_regimes.py run through the helper alone -- their inputs meet the conditions the GPU
module's tolerances were set for (cond(S) <= 1e3 at every step), and the route each step expects (kept rows, kept columns,
rows placed from V^T) follows from the library's documented rules, so the case table is self-consistent without a device:

    kept rows     first changed row // 128 * 128 against the state factored last (0 after new hyper-parameters)
    kept columns  the same against the state the candidates were solved for last; 0 when the candidate list, the semantics or
                  the hyper-parameters changed, when either solve has extra_var, or when a candidate changed kind in any way
                  other than ordinary -> unit row behind the kept columns
    counter 1     0, or every row from the first changed one to the end of the padded factor (a gather places the padding rows too)

The GPU module compares no pick (it compares the utilities of every candidate), so no top-two gap is asserted here.
"""
import numpy as np
import pytest

import incremental_forms as F
import test_fit_regimes as FR
from oracle import gp_oracle as O


def test_inputs_are_drawn_as_the_fit_regimes_draw_them():
    for N, D in ((300, 1), (1036, 2), (1036, 3), (900, 8)):
        assert F.side(N, D) == FR._side(N, D)
    assert (F.OUTPUTSCALE, F.NOISE) == (FR.OUTPUTSCALE, FR.NOISE)
    for m in F.MODELS:
        model, x, _ = F.problem(m, 100)
        ls = np.exp(model.log_ls[:F.MODELS[m][2]])
        assert np.all(ls >= 0.8) and np.all(ls <= 2.1) and x.shape == (F.FRESH + 100 + F.HELD, model.D)


def test_helper_against_posterior_chol():
    """No repeated sites, predictive semantics: S, alpha, log det, mean and variance are O.posterior_chol's."""
    for mname in ('rbf2', 'matern3'):
        model, x, truth = F.problem(mname, 100)
        rng = np.random.RandomState(3)
        idx = rng.permutation(F.FRESH)[:150]
        cand = np.arange(F.FRESH, F.FRESH + 100)
        st = dict(idx=idx, y=truth[idx] + 0.1 * rng.standard_normal(150), var=rng.choice([0.01, 0.05], 150), cand=cand, pin=False,
                  extra=None, alive=None, mean=None)
        held = np.arange(F.FRESH + 100, len(x))
        r = F.reference(model, x, st, held)
        o = O.posterior_chol(model.hypers(), x[idx], st['y'], x[np.r_[cand, held]], st['var'])
        assert np.max(np.abs(r['mu'] - o['mu'][:100])) < 1e-12 and np.max(np.abs(r['var'] - o['var'][:100])) < 1e-12
        assert np.max(np.abs(r['held'] - o['mu'][100:])) < 1e-12
        assert np.max(np.abs(r['alpha'] - o['alpha'])) < 1e-10 and abs(r['logdet'] - o['logdet']) < 1e-10
        f0, g = O.mll_and_grad(model.hypers(), x[idx], st['y'], st['var'])
        assert abs(r['mll'] - 150 * f0) < 1e-9
        assert np.max(np.abs(r['grad']() - 150 * np.r_[g['log_lengthscale'], g['log_outputscale'], g['log_noise']])) < 1e-9
        # the same state with extra_var and under greedy semantics: only the prior term moves
        e = np.linspace(0.01, 0.03, 100)
        r2 = F.reference(model, x, dict(st, pin=True, extra=e))
        assert np.allclose(r2['var'], r['var'] + e + F.NOISE, rtol=0, atol=1e-13) and np.array_equal(r2['mu'], r['mu'])


def test_scores_against_greedy_fast():
    """Greedy semantics: the first pick's utilities of O.greedy_fast, unit rows (mobile-sampled candidates) and masked rows
    included."""
    model, x, _ = F.problem('rbf2', 100)
    rng = np.random.RandomState(4)
    sub = rng.permutation(len(x))[:90]
    C = model.K(x[sub]) + F.NOISE * np.eye(90)
    static, mobile = np.zeros(90, bool), np.zeros(90, bool)
    static[:25] = True
    mobile[20:40] = True                                    # 20..24: both
    _, ut = O.greedy_fast(C, static, mobile, F.S_STD, F.M_STD, 1, 'entropy')
    A = np.where(static | mobile)[0]
    vf = 1.0 / (1.0 / F.S_STD ** 2 + 1.0 / F.M_STD ** 2)
    var = np.where(static[A] & mobile[A], vf, np.where(static[A], F.S_STD ** 2, F.M_STD ** 2))
    cand = np.where(~static)[0]
    alive = np.arange(len(cand)) % 4 != 2
    st = dict(idx=sub[A], y=np.zeros(len(A)), var=var, cand=sub[cand], pin=True, extra=None, alive=alive, mean=None)
    r = F.reference(model, x, st)
    assert np.array_equal(r['kind'] >= 0, mobile[cand])
    assert np.all(np.isneginf(r['scores'][~alive])) and not np.any(np.isnan(r['scores']))
    assert np.max(np.abs(r['scores'][alive] - ut[0][cand][alive])) < 1e-12


def test_a_second_row_of_a_site_shares_the_sites_noise():
    model, x, truth = F.problem('rbf2', 100)
    idx = np.array([3, 9, 3, 11, 3])
    r = F.reference(model, x, dict(idx=idx, y=truth[idx], var=np.full(5, 0.05)))
    S = r['S']
    assert S[0, 2] == S[2, 4] == F.OUTPUTSCALE + F.NOISE and S[0, 0] == F.OUTPUTSCALE + F.NOISE + 0.05
    assert abs(S[0, 1] - model.K(x[[3]], x[[9]])[0, 0]) < 1e-15 and S[0, 1] < F.OUTPUTSCALE


_kinds = F.kinds


def _rule_cols(vt, cur):
    if vt is None or vt['model'] is not cur['model'] or vt['pin'] != cur['pin'] or vt['extra'] is not None or \
            cur['extra'] is not None or not np.array_equal(vt['cand'], cur['cand']):
        return 0
    keep = F.first_changed_row(vt, cur) // F.NB * F.NB
    for was, now in zip(_kinds(vt), _kinds(cur)):
        if was != now and not (was < 0 and now >= keep) and not (was >= keep and now >= keep):
            return 0
    return keep


# (sequence, N of the step) -> the reason its counter is 0: the branch the step is named for, and no earlier check
WHY = {('refusal_first_row_not_in_front_of_p0', 301): 'k >= p0', ('second_readings', 310): 'no candidate',
       ('second_reading_predictive_is_solved_not_gathered', 304): 'predictive second reading',
       ('fallbacks', 306): 'no candidate', ('fallbacks', 311): 'candidate list', ('fallbacks', 316): 'hyper-parameters',
       ('fallbacks', 321): None, ('short_rbf1', 210): 'no candidate', ('solve_route', 457): 'no V^T'}


@pytest.mark.parametrize('name', sorted(F.SEQUENCES))
def test_sequence_inputs_and_expected_routes(name):
    seq = F.states(name)
    model, x, _ = F.problem(F.SEQUENCES[name]['model'], F.SEQUENCES[name]['M'])
    held = np.arange(len(x) - F.HELD, len(x))
    fact = vt = None
    worst = 0.0
    for st, expect in seq:
        N = len(st['idx'])
        assert 1 <= N <= 700 and (st['cand'] is None or len(st['cand']) <= 600)
        assert not set(map(int, st['idx'])) & set(map(int, held))
        r = F.reference(st['model'], x, st, held)
        worst = max(worst, r['cond'])
        assert r['cond'] <= 1e3, (name, N, r['cond'])
        if st['cand'] is not None:
            assert not np.any(np.isnan(r['scores'])), 'a unit row whose utility is undefined'
            assert np.array_equal(np.isnan(r['mu']), r['kind'] >= 0)
        if expect is not None:
            same_model = fact['model'] is st['model']
            p0 = F.first_changed_row(fact, st) if same_model else 0
            assert expect['kept'] == p0 // F.NB * F.NB, (name, N, p0)
            npad = (N + F.NB - 1) // F.NB * F.NB
            if expect['kept'] == 0:
                assert expect['vt'] is None
            else:
                # the gather places every row from p0 on, or the library's own checks name a reason why it cannot
                why = F.gather_refusal(vt, fact, st)
                print('%s step to N = %d: %s' % (name, N, why or 'gathered'))
                assert expect['vt'] == (npad - p0 if why is None else 0), (name, N, p0, why)
                assert why == WHY.get((name, N), why), (name, N, why)
            if st['solve']:
                assert expect['cols'] == _rule_cols(vt, st), (name, N)
            else:
                assert expect['cols'] is None
        fact = st
        if st['solve']:
            vt = st
    print('%s: largest cond(S) %.1f' % (name, worst))


def test_every_named_branch_is_in_the_table():
    """The steps the GPU module relies on to reach a branch do reach it, by the rules above."""
    S = F.SEQUENCES
    # a second reading whose first row lies in block 0, at keep - 1, in [keep, p0); a third reading
    st = F.states('second_readings')
    first, after, third = st[0][0], st[1][0], st[2][0]
    assert [int(np.sum(after['idx'] == first['idx'][k])) for k in (5, 255, 280)] == [2, 2, 2]
    assert int(np.sum(third['idx'] == first['idx'][5])) == 3
    # the refusal k >= p0: every row from p0 = 290 on is a resident candidate, row 290 an ordinary one, row 291 unchanged
    r0, r1 = (s for s, _ in F.states('refusal_first_row_not_in_front_of_p0'))
    assert F.first_changed_row(r0, r1) == 290 and set(map(int, r1['idx'][290:])) <= set(map(int, r1['cand']))
    assert _kinds(r0)[list(r1['cand']).index(r1['idx'][290])] == -1 and _kinds(r0)[list(r1['cand']).index(r1['idx'][291])] == 291
    assert r0['idx'][291] == r1['idx'][291] and r0['var'][291] == r1['var'][291]
    assert F.gather_refusal(r0, r0, r1) == 'k >= p0'
    # two rows of a site that was no train site before
    tw = st[4][0]
    assert tw['idx'][-1] == tw['idx'][-2] and int(np.sum(st[3][0]['idx'] == tw['idx'][-1])) == 0
    # exactly MAX_APPEND rows in one step; a step that passes the tight factor's leading dimension
    g = F.states('gather_scratch')
    assert len(g[2][0]['idx']) - len(g[1][0]['idx']) == 128 and len(g[2][0]['idx']) > 384 >= len(g[1][0]['idx'])
    # candidates that become unit rows behind the kept columns, a shrink that makes unit rows ordinary again
    c = F.states('carried_sums')
    k2, k3, k5, k6 = (np.array(_kinds(c[i][0])) for i in (2, 3, 5, 6))
    assert np.sum((k2 < 0) & (k3 >= 384)) == 10 and np.sum((k5 >= 384) & (k6 < 0)) == 15
    assert [e['vt'] for _, e in F.states('fallbacks')[1:]] == [0, 0, None, 0, 68]
    assert set(S) >= {'short_' + m for m in F.MODELS if m != 'rbf2'}


def test_factorize_from_script_inputs_and_kept_rows():
    """The states of the GPU module's factorize_from case: cond(S) <= 1e3, and the kept rows of every call follow from the 128-row
    rule against what the called context factored last (algp_factorize_from keeps the destination's own unchanged rows)."""
    x, held, steps = F.factorize_from_script()
    last = {'source': None, 'dest': None}
    for what, st, kept in steps:
        assert F.reference(st['model'], x, st, held)['cond'] <= 1e3
        who = 'source' if what == 'source' else 'dest'
        prev = last[who]
        assert kept == (0 if prev is None else F.first_changed_row(prev, st) // F.NB * F.NB), (what, len(st['idx']))
        if what == 'adopt':
            src = last['source']
            assert np.array_equal(src['idx'], st['idx']) and np.array_equal(src['var'], st['var'])
        last[who] = st
    assert [k for _, _, k in steps] == [0, 0, 128, 128, 128, 256, 128, 256]
