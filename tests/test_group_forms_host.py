"""CPU checks of what tests/test_group_posterior.py relies on: the reference of tests/group_forms.py has the posterior's mean
and covariance (against oracle.gp_oracle.posterior_chol, an independent Cholesky form), its aggregates reduce to them for
singleton groups, its covariance gives the variance of a contrast, and the groupings are what the GPU cases say they are."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(REPO, 'tests') not in sys.path:
    sys.path.insert(0, os.path.join(REPO, 'tests'))

import group_forms as GF                             # noqa: E402
import matern_forms as MF                            # noqa: E402
import pathwise_forms as PF                          # noqa: E402
from oracle import gp_oracle as O                    # noqa: E402

PROBLEMS = {'grid': PF.grid_problem, 'random3': lambda: PF.random_problem(3), 'random5': lambda: PF.random_problem(5),
            'duplicates': GF.duplicate_problem}


@pytest.mark.parametrize('name', list(PROBLEMS))
@pytest.mark.parametrize('kid', GF.KIDS, ids=GF.KNAMES)
def test_moments_equal_the_oracle(name, kid):
    """mu and Sigma against oracle.gp_oracle.posterior_chol to 1e-10 absolute (os = 1) for the two kernels the oracle has; for
    Matern-1/2 and Matern-5/2 against tests/matern_forms.py's posterior (mean and diagonal), which the oracle's form is held
    to by tests/test_matern_forms_host.py."""
    p = PROBLEMS[name]()
    mu, Sigma = GF.problem_moments(p, kid)
    extra = getattr(p, 'extra', None)
    assert np.array_equal(Sigma, Sigma.T) or np.max(np.abs(Sigma - Sigma.T)) < 1e-13
    if kid in (MF.RBF, MF.MATERN15):
        hyp = O.Hypers(p.log_ls, p.log_os, p.log_noise, O.KERNEL_RBF if kid == MF.RBF else O.KERNEL_MATERN15)
        ref = O.posterior_chol(hyp, p.X[p.A], p.y, p.X[p.cand], p.var, extra, want_cov=True)
        e_mu, e_cov = float(np.max(np.abs(mu - ref['mu']))), float(np.max(np.abs(Sigma - ref['cov'])))
    else:
        m, v = MF.posterior(kid, p.log_ls, p.log_os, p.log_noise, p.X[p.A], p.y, p.var, p.X[p.cand])
        e_mu = float(np.max(np.abs(mu - m)))
        e_cov = float(np.max(np.abs(np.diag(Sigma) - (v + (0.0 if extra is None else extra)))))
    print('%s kernel %d: mean %.3g covariance %.3g' % (name, kid, e_mu, e_cov))
    assert e_mu <= 1e-10 and e_cov <= 1e-10


def test_singleton_groups_reproduce_the_moments():
    p, kid = GF.duplicate_problem(), MF.MATERN25
    mu, Sigma = GF.problem_moments(p, kid)
    M = len(mu)
    for weight in (None, np.ones(M)):
        mean, cov, cross = GF.reference(p, kid, np.arange(M), weight, M)
        assert np.array_equal(mean, mu) and np.array_equal(cov, Sigma) and np.array_equal(cross, Sigma)
    # the duplicates are fully correlated up to their own extra variance
    assert abs(Sigma[0, 100] - (Sigma[0, 0] - p.extra[0])) < 1e-12


def test_contrast_variance():
    """c^T cov c of group means is the variance of the same contrast written over the sites."""
    p, kid = PF.grid_problem(), MF.RBF
    mu, Sigma = GF.problem_moments(p, kid)
    lab, Q = GF.grouping('a')
    mean, cov, cross = GF.reference(p, kid, lab, None, Q)
    c = np.zeros(Q)
    c[3], c[4] = 1.0, -1.0                                    # group 3 above group 4?
    w = np.zeros(len(mu))
    w[lab == 3] = 1.0 / np.sum(lab == 3)
    w[lab == 4] = -1.0 / np.sum(lab == 4)
    assert abs(c @ mean - w @ mu) < 1e-12
    assert abs(c @ cov @ c - w @ Sigma @ w) < 1e-12
    assert np.max(np.abs(c @ cross - w @ Sigma)) < 1e-12
    assert c @ cov @ c > 0


def test_groupings():
    lab, Q = GF.grouping('a')
    assert Q == 6 and list(np.bincount(lab[lab >= 0])) == GF.SIZES_A and np.sum(lab == -1) == 16 and lab.dtype == np.int32
    assert np.any(np.diff(np.nonzero(lab == 3)[0]) > 1)      # not contiguous
    lab, Q = GF.grouping('b')
    assert Q == 150 and np.all(np.bincount(lab) == 2)
    lab, Q = GF.grouping('c')
    assert Q == 1 and np.all(lab == 0)
    p = GF.big_problem()
    assert len(p.A) == 300 and len(p.cand) == 2600 and len(np.intersect1d(p.cand, p.A)) == 10
    assert MF.factors_in_fp32(PF.train_matrix(p, MF.RBF)) and MF.factors_in_fp32(PF.train_matrix(p, MF.MATERN05))
    lab, w, Q = GF.weighted_grouping()
    n = np.bincount(lab[lab >= 0], minlength=Q)
    assert Q == 40 and list(n) == GF.SIZES_W and n[GF.EMPTY_W] == 0 and n.max() == 700 and n.sum() <= 2600
    assert np.array_equal(w, GF.f32(w)) and np.all(np.abs(w) <= 1) and np.sum(w[lab >= 0] == 0) >= 8
    mean, cov, cross = GF.reference(p, MF.RBF, lab, w, Q)
    assert mean[GF.EMPTY_W] == 0 and not cov[GF.EMPTY_W].any() and not cov[:, GF.EMPTY_W].any() and not cross[GF.EMPTY_W].any()
    d = GF.duplicate_problem()
    assert np.array_equal(d.cand[100:105], d.cand[:5]) and len(np.unique(d.cand)) == 295
