"""The state behind algp_factorize_update / algp_solve_candidates_update / algp_factorize_from in NumPy fp64, from a plain
description of that state, and the scripted sequences of states that tests/test_incremental_forms_host.py (CPU) and
tests/test_incremental_regimes.py (GPU) share.  No device, nothing of the library.

A state is (model, pool x, train index list with repeats allowed, y, var, candidate list, prior_includes_noise, extra_var,
alive, constant mean).  `reference` returns

    S        K[A, A] + sigma_n^2 E + diag(var), E_ij = 1 where rows i and j are one pool site (the rule algp_set_train documents:
             the likelihood noise belongs to the site, var to the measurement); O.kernel_matrix / O.same_site for RBF and
             Matern-3/2, tests/matern_forms.py, additive_forms.py and relationship_forms.py for the other forms
    L, logdet, alpha = S^-1 (y - mean), mll, cond(S)
    mu, var  at the ORDINARY candidates (NaN at a unit row): mean + V' z and K_jj (+ sigma_n^2 under prior_includes_noise)
             + extra_var - |V_j|^2, V = L^-1 K[A, cand]
    scores   first-pick entropy utility of every candidate (the closed form O.greedy_fast implements, which the host test holds
             against it): CONST + 1/2 log(var_j + ss) at an ordinary row; 1/2 log1p(delta [S^-1]_kk) at a candidate that is train
             row k (its FIRST row) under prior_includes_noise; -inf where `alive` is False
    held     posterior mean at the held-out sites
    grad()   d MLL / d log-parameters (O.mll_and_grad(..., sites=...) for RBF and Matern-3/2, the forms otherwise)
    ai()     tests/ai_forms.py's average-information matrix

Inputs are drawn as tests/test_fit_regimes.py draws them: x ~ U(0, side)^D at its point density (the pool's, so that the
train set is never denser), length-scales ~ U(0.8, 2.1), outputscale 0.9, noise 0.05, var from {0.01, 0.05}; a train row whose
site is a candidate carries the mobile reading's variance 1.0, as in the agent loop -- the unit row's utility is defined for
that variance (1 + delta [S^-1]_kk > 0 needs [S^-1]_kk < 1 / 0.99).

A sequence (SEQUENCES) is: a model, N0 first rows, M candidates (0: none), prior_includes_noise, the positions among the first
rows that are candidate sites, how the first state is computed ('update': through the incremental entry points, which reserve
12.5 % headroom; 'scratch': algp_factorize / algp_solve_candidates, tight buffers that the next growth re-allocates), and steps
(ops, expect).  Ops:

    ('new', n)     append n sites that are no candidates           ('cand', n)   append the next n ordinary candidates (var 1.0)
    ('again', k)   another row (var 1.0) of the site of train row k  ('twice',)    a new candidate site, two rows at once
    ('var', k)     the other value of {0.01, 0.05} at row k         ('swap', i, j)  ('y', k)  ('cut', n) keep the first n rows
    ('drop_cand',) the candidate list loses its last entry          ('hyp',)      other length-scales
    ('replace', k) row k goes to the next ordinary candidate site (var 1.0)
    ('extra', b)   extra_var on / off   ('alive', b)  every third candidate masked / none   ('nosolve',) no candidate solve
expect: kept (rows algp_factorize_update reports), cols (columns algp_solve_candidates_update reports; None: no solve),
vt (algp_debug_counter 1, the rows placed from V^T -- padding rows of the last tile included; None: not defined, nothing kept).
"""
import functools
import zlib

import numpy as np
from scipy.linalg import solve_triangular

import additive_forms as AF
import ai_forms as AIF
import matern_forms as MF
import relationship_forms as RF
from oracle import gp_oracle as O

NB = 128
OUTPUTSCALE, NOISE = 0.9, 0.05
S_STD, M_STD = 0.1, 1.0
HELD = 16
FRESH = 720                                        # pool sites that are neither candidates nor held out


def side(N, D):
    """tests/test_fit_regimes.py's _side: the box in which N points have its point density."""
    return 2.0 * (N / 4.0) ** (1.0 / D) if D <= 2 else (27000.0 * N / 1400.0) ** (1.0 / D)


class Model(object):
    """family 'single' (spec = kernel id), 'additive' (kernel_a, kernel_b, split), 'relationship' (kernel_a, G, Q); D: the
    pool's width; explicit: the pool is handed to the library as the covariance K + sigma_n^2 I."""

    def __init__(self, name, family, spec, D, log_ls, log_os, explicit=False):
        self.name, self.family, self.spec, self.D, self.explicit = name, family, spec, D, explicit
        self.log_ls, self.log_os, self.log_noise = np.asarray(log_ls, np.float64), log_os, float(np.log(NOISE))
        self.noise = NOISE

    @property
    def theta(self):
        return AIF.pack(self.log_ls, self.log_os, self.log_noise)

    def hypers(self):
        return O.Hypers(self.log_ls, self.log_os, self.log_noise, self.spec)

    def oracle_kernel(self):
        return self.family == 'single' and self.spec in (MF.RBF, MF.MATERN15)

    def K(self, x1, x2=None):
        if self.oracle_kernel():
            return O.kernel_matrix(self.hypers(), x1, x2)
        if self.family == 'single':
            return MF.kernel_matrix(self.spec, self.log_ls, self.log_os, x1, x2)
        F = AF if self.family == 'additive' else RF
        return F.kernel_matrix(self.spec, self.log_ls, self.log_os, x1, x2)

    def prior(self, x):
        if self.family == 'relationship':
            return RF.prior_var(self.spec, self.log_os, x)
        return np.full(len(x), float(np.sum(np.exp(self.log_os))))

    def with_lengthscales(self, log_ls):
        return Model(self.name, self.family, self.spec, self.D, log_ls, self.log_os, self.explicit)


# name -> (family, spec, spatial width): D = 1, 3, 5, 8 alternate RBF and Matern-3/2 as test_fit_regimes.py's SWEEP does
MODELS = {
    'rbf2': ('single', MF.RBF, 2), 'rbf1': ('single', MF.RBF, 1), 'matern3': ('single', MF.MATERN15, 3),
    'rbf5': ('single', MF.RBF, 5), 'matern8': ('single', MF.MATERN15, 8), 'matern05': ('single', MF.MATERN05, 2),
    'matern25': ('single', MF.MATERN25, 2), 'additive': ('additive', (MF.MATERN15, MF.RBF, 2), 2),
    'relationship': ('relationship', MF.MATERN15, 2), 'cov': ('single', MF.RBF, 2),
}
N_GENO = 12


@functools.lru_cache(maxsize=None)
def problem(mname, M):
    """(model, x, truth): the pool of FRESH + M + HELD sites -- fresh ones first, then the candidates, then the held-out ones --
    and the noiseless field.  Computed once per (model, M), never written to."""
    family, spec, Ds = MODELS[mname]
    rng = np.random.RandomState(1000 * sorted(MODELS).index(mname) + M)
    P = FRESH + M + HELD
    x = rng.uniform(0, side(P, Ds), (P, Ds))
    log_ls = np.log(rng.uniform(0.8, 2.1, Ds))
    log_os = float(np.log(OUTPUTSCALE))
    D = Ds
    if family == 'additive':                       # a covariate beside the two spatial columns
        x = np.c_[x, rng.uniform(0, 24.0, P)]
        log_ls, log_os, D = np.r_[log_ls, 0.0], (float(np.log(0.6)), float(np.log(0.3))), 3
    if family == 'relationship':                   # the last column is the genotype id
        x = np.c_[x, rng.randint(0, N_GENO, P).astype(np.float64)]
        spec, log_os, D = (spec, RF.marker_relationship(Q=N_GENO, m=40), N_GENO), (float(np.log(0.6)), float(np.log(0.3))), 3
    truth = 2.0 + np.sin(x[:, 0])
    x.setflags(write=False)
    truth.setflags(write=False)
    return Model(mname, family, spec, D, log_ls, log_os, explicit=mname == 'cov'), x, truth


def reference(model, x, st, held=None):
    """The quantities of the module docstring for state `st` (a dict: idx, y, var, cand, pin, extra, alive, mean)."""
    idx, y, var = np.asarray(st['idx'], np.int64), np.asarray(st['y'], np.float64), np.asarray(st['var'], np.float64)
    N = len(idx)
    xa = x[idx]
    S = model.K(xa) + model.noise * O.same_site(idx, N) + np.diag(var)
    ev = np.linalg.eigvalsh(S)
    L = np.linalg.cholesky(S)
    mean = float(y.mean()) if st.get('mean') is None else float(st['mean'])
    z = solve_triangular(L, y - mean, lower=True)
    alpha = solve_triangular(L.T, z, lower=False)
    logdet = 2.0 * float(np.sum(np.log(np.diag(L))))
    out = dict(S=S, L=L, logdet=logdet, alpha=alpha, cond=float(ev[-1] / ev[0]), mean=mean,
               mll=float(-0.5 * z @ z - 0.5 * logdet - 0.5 * N * np.log(2.0 * np.pi)))
    cand = st.get('cand')
    if cand is not None and len(cand):
        cand = np.asarray(cand, np.int64)
        M = len(cand)
        first = {}
        for i, q in enumerate(idx):
            first.setdefault(int(q), i)
        kind = np.array([first.get(int(q), -1) if st['pin'] else -1 for q in cand], np.int64)
        B = model.K(xa, x[cand])
        for j in np.where(kind >= 0)[0]:
            B[:, j] = 0.0
            B[kind[j], j] = 1.0
        V = solve_triangular(L, B, lower=True)
        s2 = np.sum(V * V, axis=0)
        prior = model.prior(x[cand]) + (model.noise if st['pin'] else 0.0)
        if st.get('extra') is not None:
            prior = prior + np.asarray(st['extra'], np.float64)
        unit = kind >= 0
        ss, sm = S_STD ** 2, M_STD ** 2
        delta = 1.0 / (1.0 / ss + 1.0 / sm) - sm
        pv = np.where(unit, np.nan, prior - s2)
        with np.errstate(invalid='ignore'):
            ut = np.where(unit, 0.5 * np.log1p(delta * s2), O.CONST + 0.5 * np.log(pv + ss))
        if st.get('alive') is not None:
            ut = np.where(np.asarray(st['alive'], bool), ut, -np.inf)
        out.update(kind=kind, mu=np.where(unit, np.nan, mean + V.T @ z), var=pv, scores=ut)
    if held is not None:
        out['held'] = mean + model.K(x[held], xa) @ alpha
    given = st.get('mean')

    def grad():
        if model.oracle_kernel():
            _, g = O.mll_and_grad(model.hypers(), xa, y, var, mean=given, sites=idx)
            return np.r_[g['log_lengthscale'], g['log_outputscale'], g['log_noise']] * N
        return AIF.mll_and_grad(model.family, model.spec, model.theta, xa, y, var, sites=idx, mean=given)[1]

    out['grad'] = grad
    out['ai'] = lambda: AIF.average_information(model.family, model.spec, model.theta, xa, y, var, sites=idx, mean=given)
    return out


# ---- the scripted sequences -----------------------------------------------------------------------------------------------------
def E(kept, cols=None, vt=None):
    return dict(kept=kept, cols=cols, vt=vt)


def _seq(model='rbf2', N0=300, M=0, pin=True, units=(), first='update', steps=(), mean=None, shared=False):
    return dict(model=model, N0=N0, M=M, pin=pin, units=tuple(units), first=first, steps=list(steps), mean=mean, shared=shared)


def _gather(first):
    """Every new site a resident ordinary candidate: p0 = 300 in mid-block (rows [256, 300) keep what they hold), then exactly
    MAX_APPEND = 128 rows across a tile boundary; `first` = 'scratch' makes the factor and V^T grow in that call."""
    return _seq(M=300, first=first, steps=[([('cand', 40)], E(256, 256, 84)), ([('cand', 128)], E(256, 256, 172))])


def _gather_boundary(first):
    """p0 = 256 on a block boundary (keep == p0, no partial block) and a whole new padded tile; then up to N = 384 exactly."""
    return _seq(N0=256, M=300, first=first, steps=[([('cand', 40)], E(256, 256, 128)), ([('cand', 88)], E(256, 256, 88))])


def _carried(pin):
    """A fixed candidate list over appends that advance the finished column blocks (acc_cols 256 -> 384), candidates that become
    unit rows behind the kept columns with the running sums live, a re-target in block 0 (u changes from row 0: the sums must be
    rebuilt), a shrink that turns unit rows back into ordinary ones, an alive mask, extra_var on and off."""
    c = (lambda a, b: a) if pin else (lambda a, b: b)        # predictive semantics: no unit rows, a kind never changes
    return _seq(N0=370, M=300, pin=pin, units=(5, 280), steps=[
        ([('cand', 10)], E(256, 256, 14)),
        ([('cand', 10)], E(256, 256, 132)),
        ([('cand', 10)], E(384, 384, 122)),
        ([('y', 3)], E(384, 384, 112)),
        ([('cand', 10)], E(384, 384, 112)),
        ([('cut', 395)], E(384, c(0, 384), 117)),
        ([('alive', True), ('cand', 5)], E(384, 384, 117)),
        ([('alive', False), ('extra', True)], E(384, 0, 112)),
        ([('extra', False), ('cand', 3)], E(384, 0, 112))])


def _short(model):
    """Sequences 2 + 3 in their shortest form for another width, kernel or pool: the gather, then the triangular solve."""
    return _seq(model=model, N0=130, M=100, shared=True, steps=[([('cand', 40)], E(128, 128, 126)), ([('new', 40)], E(128, 128, 0))])


SEQUENCES = {
    # 1. nothing is kept below one block; the first kept block (Npad 128 -> 256 inside the headroom)
    'keep0_from_1': _seq(N0=1, steps=[([('new', 127)], E(0)), ([('new', 1)], E(128, vt=0))]),
    'keep0_from_5': _seq(N0=5, steps=[([('new', 124)], E(0))]),
    'keep0_from_127': _seq(N0=127, steps=[([('new', 1)], E(0)), ([('new', 1)], E(128, vt=0))]),
    'first_kept_block': _seq(N0=128, steps=[([('new', 1)], E(128, vt=0))]),
    # 2. the triangular solve: no candidates resident.  129 -> 130 -> 256 (ends on a boundary) -> 257 -> 457: the last append
    # passes the factor's leading dimension (384): reserve_factor copies keep_height = p0 = 257 > keep_rows = 256 rows, and u, w
    # are re-allocated (the substitutions restart at row 0); then y alone changes, in block 0 and in the last block
    'solve_route': _seq(N0=129, steps=[([('new', 1)], E(128, vt=0)), ([('new', 126)], E(128, vt=0)), ([('new', 1)], E(256, vt=0)),
                                       ([('new', 200)], E(256, vt=0)), ([('y', 3)], E(384, vt=0)), ([('y', 450)], E(384, vt=0))]),
    # the same with a constant mean that is given: z = u - mean w
    'solve_route_mean_given': _seq(N0=129, mean=1.7, steps=[([('new', 1)], E(128, vt=0)), ([('y', 3)], E(128, vt=0))]),
    # 3. the gather from V^T
    'gather_update': _gather('update'), 'gather_scratch': _gather('scratch'),
    'gather_boundary_update': _gather_boundary('update'), 'gather_boundary_scratch': _gather_boundary('scratch'),
    # 4. second readings through the gather: k = 5 in block 0, k = 255 = keep - 1, k = 280 in [keep, p0); a third reading of
    # k = 5; a change at row 200, which is no candidate site, with one more reading of k = 280 (the solve, counter 0); a site first
    # added and read twice in one step (an ordinary row of V^T at the time of the solve: both rows are gathered, the tail block
    # carries their shared noise)
    'second_readings': _seq(M=300, units=(5, 255, 280), steps=[
        ([('again', 5), ('again', 255), ('again', 280), ('cand', 3)], E(256, 256, 84)),
        ([('again', 5), ('cand', 2)], E(256, 256, 78)),
        ([('var', 200), ('again', 280)], E(128, 128, 0)),
        ([('twice',)], E(256, 256, 74))]),
    'second_readings_scratch': _seq(M=300, units=(5, 255, 280), first='scratch', steps=[
        ([('again', 5), ('again', 255), ('again', 280), ('cand', 90)], E(256, 256, 212))]),
    # the refusal k >= p0: the last ten rows are candidate sites (unit rows 290 .. 299 of V^T); row 290 is given to a NEW candidate
    # site, so p0 = 290 and every row from there on is a resident candidate -- the new site an ordinary one, gathered as it is;
    # row 291 is unchanged in site and variance, and the only reason not to take it as L[291, :] - var * unit row is that row 291
    # of L is not among the rows in front of p0 (the host test proves that this is the reason, gather_refusal)
    'refusal_first_row_not_in_front_of_p0': _seq(M=300, units=tuple(range(290, 300)), steps=[
        ([('replace', 290), ('again', 295)], E(256, 0, 0))]),
    # 5. fall-backs from the gather (counter 0): a new site that is no candidate; the candidate list changed since the solve;
    # V^T solved under other hyper-parameters; then the gather again
    'fallbacks': _seq(M=300, steps=[
        ([('new', 1), ('cand', 5)], E(256, 256, 0)),
        ([('drop_cand',), ('cand', 5)], E(256, 0, 0)),
        ([('hyp',), ('nosolve',)], E(0)),
        ([('cand', 5)], E(256, 0, 0)),
        ([('cand', 5)], E(256, 256, 68))]),
    # 6. changes inside the kept prefix, shrinks and growth after them
    'prefix_changes': _seq(shared=True, steps=[
        ([('var', 0)], E(0)), ([('var', 127)], E(0)), ([('var', 128)], E(128, vt=0)), ([('var', 290)], E(256, vt=0)),
        ([('swap', 140, 141)], E(128, vt=0)), ([('y', 3)], E(256, vt=0)), ([('y', 299)], E(256, vt=0)),
        ([('cut', 200)], E(128, vt=0)), ([('new', 100)], E(128, vt=0)), ([('cut', 256)], E(256, vt=0)),
        ([('new', 44)], E(256, vt=0))]),
    # 7. candidate columns with carried sums, greedy and predictive semantics
    'carried_sums': _carried(True), 'carried_sums_predictive': _carried(False),
    # the defect this table found: under predictive semantics V^T holds the site of train row 5 as an ORDINARY row, without the
    # sigma_n^2 that a second row of the site shares with row 5 -- gathered as it is, the new row of L is wrong (the factor was
    # 2.6e-2 of max |L| off, fp64 and fp32 alike); the update has to solve these rows (counter 0)
    'second_reading_predictive_is_solved_not_gathered': _seq(M=300, pin=False, units=(5,), steps=[([('again', 5), ('cand', 3)], E(256, 256, 0))]),
    # 9. widths, kernels, pools
    **{'short_' + m: _short(m) for m in sorted(MODELS) if m != 'rbf2'},
}


def states(name):
    """[(state, expect)] of a sequence, the first state (expect None) included.  Every state is a dict of its own arrays."""
    sq = SEQUENCES[name]
    model, x, truth = problem(sq['model'], sq['M'])
    rng = np.random.RandomState(zlib.crc32(name.encode()))               # (a new sequence leaves the others' inputs alone)
    M = sq['M']
    cand = np.arange(FRESH, FRESH + M)
    order = list(cand[rng.permutation(M)])                    # the order in which candidates join the train set
    fresh = list(rng.permutation(FRESH))
    idx, var = [], []
    for i in range(sq['N0']):
        if i in sq['units']:
            idx.append(int(order.pop(0)))
            var.append(M_STD ** 2)
        else:
            idx.append(int(fresh.pop(0)))
            var.append(float(rng.choice([0.01, 0.05])))
    noise = lambda: 0.1 * float(rng.standard_normal())
    y = [float(truth[q]) + noise() for q in idx]
    st = dict(model=model, idx=idx, var=var, y=y, cand=cand if M else None, pin=sq['pin'], extra=None, alive=None, mean=sq['mean'],
              solve=M > 0)
    snap = lambda: dict(st, idx=np.array(st['idx'], np.int64), var=np.array(st['var']), y=np.array(st['y']))
    out = [(snap(), None)]

    def add(q, v):
        st['idx'].append(int(q))
        st['var'].append(float(v))
        st['y'].append(float(truth[q]) + noise())

    for ops, expect in sq['steps']:
        st['solve'] = M > 0
        for op in ops:
            k = op[0]
            if k == 'new':
                for _ in range(op[1]):
                    add(fresh.pop(0), rng.choice([0.01, 0.05]))
            elif k == 'cand':
                for _ in range(op[1]):
                    add(order.pop(0), M_STD ** 2)
            elif k == 'again':
                add(st['idx'][op[1]], M_STD ** 2)
            elif k == 'twice':
                q = order.pop(0)
                add(q, M_STD ** 2)
                add(q, M_STD ** 2)
            elif k == 'replace':
                q = order.pop(0)
                st['idx'][op[1]], st['var'][op[1]], st['y'][op[1]] = int(q), M_STD ** 2, float(truth[q]) + noise()
            elif k == 'var':
                st['var'][op[1]] = 0.06 - st['var'][op[1]]
            elif k == 'swap':
                i, j = op[1], op[2]
                for a in (st['idx'], st['var'], st['y']):
                    a[i], a[j] = a[j], a[i]
            elif k == 'y':
                st['y'][op[1]] += 0.7
            elif k == 'cut':
                for a in ('idx', 'var', 'y'):
                    st[a] = st[a][:op[1]]
                # sites that left the train set may join it again
                order = [int(q) for q in cand[np.argsort(rng.rand(M))] if int(q) not in set(st['idx'])] if M else order
            elif k == 'drop_cand':
                st['cand'] = st['cand'][:-1]
                order = [q for q in order if q != int(cand[-1])]
            elif k == 'hyp':
                st['model'] = st['model'].with_lengthscales(np.log(np.exp(st['model'].log_ls) * 1.07))
            elif k == 'extra':
                st['extra'] = 0.02 + 0.01 * (np.arange(len(st['cand'])) % 3) if op[1] else None
            elif k == 'alive':
                st['alive'] = (np.arange(len(st['cand'])) % 3 != 1) if op[1] else None
            elif k == 'nosolve':
                st['solve'] = False
            else:
                raise ValueError(op)
        out.append((snap(), expect))
    return out


def first_changed_row(a, b):
    """The first row at which two train states differ in site or variance (the shorter one's length if none does)."""
    lim = min(len(a['idx']), len(b['idx']))
    p = 0
    while p < lim and a['idx'][p] == b['idx'][p] and a['var'][p] == b['var'][p]:
        p += 1
    return p


def kinds(st):
    """Per candidate: its site's FIRST train row under prior_includes_noise, else -1 (an ordinary row of V^T)."""
    first = {}
    for i, q in enumerate(st['idx']):
        first.setdefault(int(q), i)
    return [first.get(int(q), -1) if st['pin'] else -1 for q in st['cand']]


def gather_refusal(vt, fact, cur):
    """Why algp_factorize_update cannot take the new rows of `cur` from the V^T solved for state `vt` (None: it can), `fact`
    being the state factored last: the checks of vt_rows_for_new_sites (api_factor.hip) in their order."""
    p0 = first_changed_row(fact, cur)
    Nb = p0 // NB * NB
    if vt is None or vt['cand'] is None:
        return 'no V^T'
    if vt['model'] is not cur['model']:
        return 'hyper-parameters'
    if len(vt['idx']) < Nb or first_changed_row(vt, cur) < Nb:
        return 'V^T solved for other kept rows'
    if not np.array_equal(vt['cand'], cur['cand']):
        return 'candidate list'
    pos = {int(q): j for j, q in enumerate(cur['cand'])}
    vk = kinds(vt)
    first = {}
    for i, q in enumerate(cur['idx']):
        first.setdefault(int(q), i)
    for i in range(p0, len(cur['idx'])):
        q = int(cur['idx'][i])
        if q not in pos:
            return 'no candidate'
        k = vk[pos[q]]
        if k >= 0:
            if k >= p0:
                return 'k >= p0'
            if cur['idx'][k] != q or len(vt['idx']) <= k or vt['idx'][k] != q or vt['var'][k] != cur['var'][k]:
                return 'row k changed'
        elif first[q] < Nb:
            return 'predictive second reading'
    return None


@functools.lru_cache(maxsize=None)
def factorize_from_script():
    """algp_factorize_from from a source that grows 129 -> 257 -> 300 by updates (zero targets: the greedy context) into a
    destination that holds nothing, a shorter prefix, then a longer factor (350 rows) whose tail differs from row 200 on; at last
    only the destination's y changes.  (x, held, steps); a step is ('source', state, kept): the source's update; ('adopt', state,
    kept): set_train + factorize_from in the destination; ('own', state, kept): the destination's own update."""
    model, x, truth = problem('rbf2', 0)
    rng = np.random.RandomState(21)
    sites = rng.permutation(FRESH)
    idx, var = sites[:300], rng.choice([0.01, 0.05], 300)
    y = truth[idx] + 0.1 * rng.standard_normal(300)
    other = np.r_[idx[:200], sites[300:450]]
    st = lambda i, t, v: dict(model=model, idx=np.array(i), y=np.array(t), var=np.array(v), cand=None, solve=False, mean=None)
    src = lambda n: st(idx[:n], np.zeros(n), var[:n])
    dst = lambda n: st(idx[:n], y[:n], var[:n])
    y2 = y.copy()
    y2[7] += 0.7
    y2[290] -= 0.4
    steps = [('source', src(129), 0), ('adopt', dst(129), 0), ('source', src(257), 128), ('adopt', dst(257), 128),
             ('own', st(other, truth[other], np.r_[var[:200], np.full(150, 0.05)]), 128), ('source', src(300), 256),
             ('adopt', dst(300), 128), ('own', st(idx, y2, var), 256)]
    return x, np.arange(len(x) - HELD, len(x)), steps
