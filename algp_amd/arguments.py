"""Command-line flags of the reference (reference arguments.py:7-52), same names and defaults.
Differences: `--kernel` accepts {rbf, matern, additive, separable, genotype} only, and `--matern_nu` {0.5, 1.5, 2.5} picks the Matern form
(the reference fixes nu in its source, models.py:219-222); `--kernel additive` is the sum of `--kernel_a` over the first
`--kernel_split` coordinates and `--kernel_b` over the others (`--matern_nu` applies to its Matern parts); `--kernel genotype` is
`--kernel_a` (with `--matern_nu`) over the position plus a genotype effect per id in the last coordinate, with the relationship
matrix of `--relationship PATH` (a .npy file) or independent genotypes without it; `--kernel separable` is the product of
`--kernel_a` over the first `--kernel_split` coordinates and `--kernel_b` over the others with one outputscale (`--matern_nu 0.5`
with both parts matern and split 1: AR1 x AR1), and `--kernel genotype --spatial separable` puts AR1(row) x AR1(col) -- Matern-1/2
over the row times Matern-1/2 over the column, whatever `--kernel_a` says -- in the place of the genotype kernel's spatial part;
`--fit_method ai` fits by average-information
Newton steps instead of Adam; `--dtype`/`--device` select the GPU precision
and card; no results directory is created and nothing prompts (the reference's interactive
`input()` at arguments.py:41-49 blocks unattended runs)."""
import argparse

import numpy as np


def get_parser():
    p = argparse.ArgumentParser(description='Adaptive Sampling and Informative Planning (MI355X GP path)')
    p.add_argument('--lr', default=.1, type=float)
    p.add_argument('--max_iterations', default=200, type=int)
    p.add_argument('--fit_method', default='adam', choices=['adam', 'ai'],
                   help="GPR.fit: the reference's Adam loop, or damped Newton steps on the average-information matrix "
                        '(--max_iterations then caps the MLL evaluations)')
    p.add_argument('--fixed_effects', default='none', choices=['none', 'intercept', 'linear'],
                   help='fixed effects of the mean, estimated by generalised least squares: the constant, or the constant and '
                        'a linear trend in every coordinate (predictions then carry the trend and its uncertainty)')
    p.add_argument('--fit_objective', default='mll', choices=['mll', 'reml'],
                   help="GPR.fit's objective: the marginal likelihood of y - mean(y), or the restricted likelihood of the fixed "
                        "effects (with --fixed_effects none: of the intercept)")
    p.add_argument('--data_file', default=None)
    p.add_argument('--phenotype', default='plant_height')
    p.add_argument('--kernel', default='matern', choices=['rbf', 'matern', 'additive', 'separable', 'genotype'])
    p.add_argument('--matern_nu', default=1.5, type=float, choices=[0.5, 1.5, 2.5])
    p.add_argument('--kernel_split', default=2, type=int, help='additive and separable kernels: coordinates [0, split) belong to part a')
    p.add_argument('--kernel_a', default='matern', choices=['rbf', 'matern'], help='additive and separable kernels: form of part a')
    p.add_argument('--kernel_b', default='rbf', choices=['rbf', 'matern'], help='additive and separable kernels: form of part b')
    p.add_argument('--spatial', default='single', choices=['single', 'separable'],
                   help="genotype kernel: its spatial part is --kernel_a over the position, or the separable AR1(row) x AR1(col) "
                        "(Matern-1/2 over the row times Matern-1/2 over the column)")
    p.add_argument('--relationship', default=None, help='genotype kernel: .npy file with the Q x Q relationship matrix (default: identity)')
    p.add_argument('--latent', default=None)
    p.add_argument('--num_sims', default=10, type=int)
    p.add_argument('--num_runs', default=6, type=int)
    p.add_argument('--fraction_pretrain', default=.75, type=float)
    p.add_argument('--num_samples_per_batch', default=4, type=int)
    p.add_argument('--slack', default=0, type=int)
    p.add_argument('--num_test', default=40, type=int)
    p.add_argument('--update', action='store_true')
    p.add_argument('--update_every', default=1, type=int)
    p.add_argument('--criterion', default='entropy', choices=['entropy', 'mutual_information', 'variance_reduction'])
    p.add_argument('--static_std', default=.1, type=float)
    p.add_argument('--render', action='store_true')
    p.add_argument('--seed', default=1, type=int)
    p.add_argument('--id', default=1, type=int)
    p.add_argument('--save_dir', default='results')
    p.add_argument('--eval_only', action='store_true')
    p.add_argument('--dtype', default='float64', choices=['float32', 'float64'])
    p.add_argument('--device', default=0, type=int)
    p.add_argument('--rows', default=20, type=int, help='synthetic field rows')
    p.add_argument('--cols', default=20, type=int, help='synthetic field columns')
    return p


def get_args(argv=None):
    args = get_parser().parse_args(argv)
    args.dtype = np.dtype(args.dtype)
    return args
