#!/usr/bin/env python
"""Demo driver for the GP path (BASELINE config 1: `python run.py --eval_only`, a 20 x 20 synthetic
mixture-of-Gaussians field).  It mirrors the reference's run_demo flow (reference run.py:207-219)
minus the networkx path planner: pre-train the GP on a pilot survey, then per batch greedily pick
the most informative static sites, sample them, (optionally) refit, and predict the held-out set.
Needs an MI355X: there is no CPU path."""
import time

import numpy as np

from algp_amd.agent import Agent
from algp_amd.arguments import get_args
from algp_amd.field import SyntheticField
from algp_amd.utils import compute_mae


def run_demo(args):
    np.random.seed(args.seed)
    # an additive kernel whose first part is the whole position (row, col) needs a coordinate for its second: genotype ids
    # (the genotype kernel reads the ids from the same column)
    genotypes = 12 if (args.kernel == 'additive' and args.kernel_split == 2) or args.kernel == 'genotype' else 0
    # the separable kernel over (row | col) gets a field drawn from AR1(row) x AR1(col): the demo fits what generated it
    separable = (args.kernel == 'separable' and args.kernel_split == 1) or (args.kernel == 'genotype' and args.spatial == 'separable')
    env = SyntheticField(args.rows, args.cols, num_test=args.num_test, num_genotypes=genotypes, ar1=(0.8, 0.6) if separable else None)
    agent = Agent(env, args, static_std=args.static_std, mobile_std=10 * args.static_std)
    agent.reset()
    agent._setup_ipp(args.criterion, args.update)
    errors = []
    for i in range(args.num_runs):
        t0 = time.time()
        picks = agent.greedy(args.num_samples_per_batch)
        agent._add_samples(picks, [agent.static_std] * len(picks))
        if args.update and (i + 1) % args.update_every == 0:
            agent.update_model()
            agent._post_update()
        pred, var = agent.predict(return_var=True)
        err = compute_mae(env.test_Y, pred)
        errors.append(err)
        print('Run {}/{}: picks {} test ERROR {:.4f} predictive variance max {:.3f} min {:.3f} mean {:.3f} ({:.3f}s)'
              .format(i + 1, args.num_runs, picks, err, var.max(), var.min(), var.mean(), time.time() - t0))
    if agent.gp.fixed_effects is not None:
        beta, cov = agent.gp.fixed_effect_estimates()
        print('fixed effects (' + agent.gp.fit_objective + '): ' +
              '  '.join('{:+.4f} +- {:.4f}'.format(b, s) for b, s in zip(beta, np.sqrt(np.diag(cov)))))
    if separable and args.fit_method == 'ai':
        try:
            (rr, sr), (rc, sc) = agent.gp.ar1_correlations()
            print('AR1 correlations: rho_row = {:.3f} +- {:.3f}  rho_col = {:.3f} +- {:.3f}'.format(rr, sr, rc, sc))
        except ValueError:
            pass                               # a part that is no Matern-1/2 over one coordinate has no AR1 correlation
    if args.kernel == 'genotype':
        # the genotype effects themselves, beside the simulated ones (both centred: the constant mean absorbs their average)
        mean, var = agent.gp.genotype_effects()
        sim = env.genotype_effect - env.genotype_effect.mean()
        print('genotype   fitted effect  (sd)     simulated')
        for q in range(len(mean)):
            print('{:8d}   {:+.4f}  ({:.4f})   {:+.4f}'.format(q, mean[q] - mean.mean(), np.sqrt(max(var[q], 0.0)), sim[q]))
        if args.fit_method == 'ai':
            h2, se = agent.gp.heritability()
            print('heritability h2 = {:.3f} +- {:.3f}'.format(h2, se))
    return errors


if __name__ == '__main__':
    run_demo(get_args())
