"""GP model wrapper with the reference's `GPR` surface (reference models.py:86-203), backed by
libalgp_hip.so instead of GPyTorch.

Same constructor, methods, properties and parameter names as the reference so that its callers
(agent.py:34-45, 84-90; utils.py:296-298; run.py:35-37) work unchanged:

    gp = GPR(latent=None, lr=.1, max_iterations=200, kernel_params={'type': 'rbf'})
    gp.fit(x, y, var); gp.cov_mat(x1, x2, white_noise_var, add_likelihood_var)
    dict(gp.model.named_parameters())['kernel_covar_module.log_outputscale']
    gp.model.state_dict() / load_state_dict()

What differs, deliberately:
  * arithmetic runs on the GPU in `dtype` (float64 by default; the reference is float32 through
    utils.py:19) -- pass dtype=np.float32 for the reference's precision;
  * only the identity latent function and the rbf / matern kernels exist, the latter with
    kernel_params['nu'] = 0.5, 1.5 (the default when 'nu' is absent) or 2.5; 'nu' is ignored for
    rbf (north_star scope; the reference also has linear / non_linear latents and a spectral
    mixture kernel, models.py:23-44, 221-223): anything else, another nu included, raises
    NotImplementedError like models.py:227, 248;
  * kernel_params = {'type': 'additive', 'split': Da, 'parts': ({'type': 'matern', 'nu': 1.5}, {'type': 'rbf'})} is the sum of
    two such kernels, the first over coordinates [0, Da), the second over the others (genotype effect + spatial trend), with
    gpytorch's AdditiveKernel parameter names: kernel_covar_module.kernels.{0,1}.log_outputscale and
    kernel_covar_module.kernels.{0,1}.base_kernel.log_lengthscale; GPR.predict_components splits the posterior mean;
  * kernel_params = {'type': 'genotype', 'spatial': {'type': 'matern', 'nu': 1.5}, 'relationship': G_or_None, 'n_genotypes': Q}
    is the relationship kernel os_a kappa_a(r_a) + os_g G[g, g'] (GBLUP with a spatial term): the LAST column of x holds the
    integer genotype ids, the others are spatial; G is a (Q, Q) relationship matrix or None for the identity.  Parameter names
    follow the additive layout: kernel_covar_module.kernels.0.base_kernel.log_lengthscale (1, 1, D - 1),
    kernel_covar_module.kernels.0.log_outputscale, kernel_covar_module.kernels.1.log_outputscale (the table is data, not a
    parameter); GPR.genotype_effects gives the BLUPs with their variances or joint covariance;
  * kernel_params = {'type': 'separable', 'split': Da, 'parts': (desc_a, desc_b)} is the PRODUCT os kappa_a(r_a) kappa_b(r_b) of two
    such kernels over the coordinates [0, Da) and the others, with one outputscale -- two Matern-1/2 parts over one coordinate
    each are AR1(row) x AR1(col) -- under gpytorch's ScaleKernel(ProductKernel(...)) names:
    kernel_covar_module.base_kernel.kernels.{0,1}.log_lengthscale and kernel_covar_module.log_outputscale.  It may also be the
    'spatial' entry of the genotype kernel, whose first part is then that ScaleKernel:
    kernel_covar_module.kernels.0.base_kernel.kernels.{0,1}.log_lengthscale, kernel_covar_module.kernels.0.log_outputscale,
    kernel_covar_module.kernels.1.log_outputscale.  GPR.ar1_correlations gives rho = exp(-spacing / ls) of its AR1 parts with
    standard errors;
  * `fit` uses the analytic MLL gradient computed on the device with the reference's own optimiser
    objects (torch.optim.Adam + ReduceLROnPlateau(patience=50), models.py:121-124);
  * GPR(..., fit_method='ai') fits by damped Newton steps on the average-information matrix of the MLL instead (utils.ai_newton,
    algp_get_mll_ai: tens of device steps, not hundreds); after either method hyper_covariance / hyper_standard_errors give the
    covariance and standard errors of the log hyper-parameters and, under the genotype kernel, heritability gives h2 with its
    standard error;
  * GPR(..., fixed_effects='intercept' | 'linear' | callable) gives the mean a linear part h(x)' beta estimated by generalised
    least squares (block, replicate and trend terms): predict returns the trend-aware mean and the variance with the
    universal-kriging term, fixed_effect_estimates the estimates and their covariance; fit_objective='reml' fits either method
    on the restricted likelihood (algp_reml_step, algp_get_reml_ai), and hyper_covariance, hyper_standard_errors and heritability
    then use its average information.  Without the two arguments every path is the one it was.
"""
import numpy as np
import torch
import torch.nn as nn

from . import _hip

_KERNELS = {None: _hip.KERNEL_RBF, 'rbf': _hip.KERNEL_RBF, 'matern': _hip.KERNEL_MATERN15}
_MATERN_NU = {0.5: _hip.KERNEL_MATERN05, 1.5: _hip.KERNEL_MATERN15, 2.5: _hip.KERNEL_MATERN25}


class IdentityLatentFunction(nn.Module):
    """models.py:15-21"""

    def __init__(self):
        super(IdentityLatentFunction, self).__init__()
        self.embed_dim = None

    def forward(self, x):
        return x


class _BaseKernel(nn.Module):
    def __init__(self, ard_num_dims):
        super(_BaseKernel, self).__init__()
        self.log_lengthscale = nn.Parameter(torch.zeros(1, 1, ard_num_dims, dtype=torch.float64))


class _ScaleKernel(nn.Module):
    def __init__(self, ard_num_dims):
        super(_ScaleKernel, self).__init__()
        self.base_kernel = _BaseKernel(ard_num_dims)
        self.log_outputscale = nn.Parameter(torch.zeros(1, dtype=torch.float64))


class _AdditiveKernel(nn.Module):
    """Two ScaleKernels, the first on the leading `split` coordinates, the second on the others (gpytorch's AdditiveKernel)."""

    def __init__(self, split, ard_num_dims):
        super(_AdditiveKernel, self).__init__()
        self.kernels = nn.ModuleList([_ScaleKernel(split), _ScaleKernel(ard_num_dims - split)])


class _ProductKernel(nn.Module):
    """Two base kernels, the first on the leading `split` coordinates, the second on the others (gpytorch's ProductKernel)."""

    def __init__(self, split, ard_num_dims):
        super(_ProductKernel, self).__init__()
        self.kernels = nn.ModuleList([_BaseKernel(split), _BaseKernel(ard_num_dims - split)])


class _ScaleProductKernel(nn.Module):
    """ScaleKernel(ProductKernel(a, b)): one outputscale for the product."""

    def __init__(self, split, ard_num_dims):
        super(_ScaleProductKernel, self).__init__()
        self.base_kernel = _ProductKernel(split, ard_num_dims)
        self.log_outputscale = nn.Parameter(torch.zeros(1, dtype=torch.float64))


class _TableKernel(nn.Module):
    """The genotype part os_g G[g, g']: its outputscale is the only parameter."""

    def __init__(self):
        super(_TableKernel, self).__init__()
        self.log_outputscale = nn.Parameter(torch.zeros(1, dtype=torch.float64))


class _GenotypeKernel(nn.Module):
    """ScaleKernel over the D - 1 spatial coordinates plus the table-valued genotype part."""

    def __init__(self, ard_num_dims, split=None):
        super(_GenotypeKernel, self).__init__()
        spatial = _ScaleKernel(ard_num_dims - 1) if split is None else _ScaleProductKernel(split, ard_num_dims - 1)
        self.kernels = nn.ModuleList([spatial, _TableKernel()])


def _separable_ids(params, n_spatial):
    """(split, id_a, id_b) of {'type': 'separable', 'split': Da, 'parts': (desc_a, desc_b)} over n_spatial coordinates."""
    parts, split = params.get('parts'), params.get('split')
    if parts is None or len(parts) != 2:
        raise ValueError("separable kernel: 'parts' must hold two kernel descriptions")
    if split is None or not 1 <= int(split) <= n_spatial - 1:
        raise ValueError("separable kernel: 'split' must be in [1, %d] (%d spatial coordinates)" % (n_spatial - 1, n_spatial))
    return int(split), _kernel_id(parts[0]), _kernel_id(parts[1])


def _kernel_id(params):
    """The library's id of a single form: {'type': 'rbf' | 'matern'[, 'nu': 0.5 | 1.5 | 2.5]} (None: rbf)."""
    kernel = params['type'] if params is not None else 'rbf'
    if kernel not in _KERNELS:
        raise NotImplementedError(kernel)
    if kernel == 'matern' and 'nu' in params:
        nu = params['nu']
        if nu not in _MATERN_NU:
            raise NotImplementedError('matern nu=%r: nu is one of 0.5, 1.5, 2.5' % (nu,))
        return _MATERN_NU[nu]
    return _KERNELS[kernel]


class _GaussianLikelihood(nn.Module):
    def __init__(self):
        super(_GaussianLikelihood, self).__init__()
        self.log_noise = nn.Parameter(torch.zeros(1, dtype=torch.float64))


class ExactGPModel(nn.Module):
    """Parameter container with the reference's names (models.py:206-254): zero mean on
    mean-centred targets, ScaleKernel(RBF-ARD | Matern-nu, nu = 1/2, 3/2, 5/2), per-point white
    noise, Gaussian likelihood.  It holds no arithmetic: the GPU library reads the parameters."""

    def __init__(self, train_x, train_y, likelihood, var=None, latent=None, kernel_params=None, latent_params=None):
        super(ExactGPModel, self).__init__()
        if latent is not None and latent != 'identity':
            raise NotImplementedError('latent function %r is outside the MI355X hot path (identity only)' % (latent,))
        self.latent_func = IdentityLatentFunction()
        kernel = kernel_params['type'] if kernel_params is not None else 'rbf'
        self.split = None
        self.relationship = None               # (G or None, Q) under the genotype kernel
        self.sep = None                        # (split, id_a, id_b) where the (spatial) kernel is the separable product
        if kernel == 'genotype':
            D = int(np.shape(train_x)[-1])
            if D < 2:
                raise ValueError('genotype kernel: x needs a spatial coordinate and the genotype id column (D >= 2)')
            G = kernel_params.get('relationship')
            Q = kernel_params.get('n_genotypes')
            if G is not None:
                G = np.ascontiguousarray(G, dtype=np.float64)
                if G.ndim != 2 or G.shape[0] != G.shape[1]:
                    raise ValueError("genotype kernel: 'relationship' must be a square matrix")
                if Q is not None and int(Q) != G.shape[0]:
                    raise ValueError("genotype kernel: 'n_genotypes' does not match 'relationship'")
                Q = G.shape[0]
            elif Q is None:
                raise ValueError("genotype kernel: pass 'relationship' or 'n_genotypes'")
            self.relationship = (G, int(Q))
            spatial = kernel_params.get('spatial')
            if spatial is not None and spatial.get('type') == 'separable':
                if D < 3:
                    raise ValueError('genotype kernel over a separable spatial part: two spatial coordinates and the id column (D >= 3)')
                self.sep = _separable_ids(spatial, D - 1)
                self.kernel_type = ('genotype', ('separable',) + self.sep)
                self.kernel_covar_module = _GenotypeKernel(D, self.sep[0])
            else:
                self.kernel_type = ('genotype', _kernel_id(spatial))
                self.kernel_covar_module = _GenotypeKernel(D)
            self.likelihood = likelihood
            return
        if kernel == 'separable':
            D = int(np.shape(train_x)[-1])
            self.sep = _separable_ids(kernel_params, D)
            self.kernel_type = ('separable',) + self.sep
            self.kernel_covar_module = _ScaleProductKernel(self.sep[0], D)
            self.likelihood = likelihood
            return
        if kernel == 'additive':
            D = int(np.shape(train_x)[-1])
            parts = kernel_params.get('parts')
            split = kernel_params.get('split')
            if parts is None or len(parts) != 2:
                raise ValueError("additive kernel: 'parts' must hold two kernel descriptions")
            if split is None or not 1 <= int(split) <= D - 1:
                raise ValueError("additive kernel: 'split' must be in [1, D - 1] (D = %d)" % D)
            self.split = int(split)
            self.kernel_type = ('additive', self.split, _kernel_id(parts[0]), _kernel_id(parts[1]))
            self.kernel_covar_module = _AdditiveKernel(self.split, D)
            self.likelihood = likelihood
            return
        if kernel not in _KERNELS:
            raise NotImplementedError(kernel)
        self.kernel_type = _KERNELS[kernel]
        if kernel == 'matern' and 'nu' in kernel_params:
            nu = kernel_params['nu']
            if nu not in _MATERN_NU:
                raise NotImplementedError('matern nu=%r: nu is one of 0.5, 1.5, 2.5' % (nu,))
            self.kernel_type = _MATERN_NU[nu]
        self.kernel_covar_module = _ScaleKernel(int(np.shape(train_x)[-1]))
        self.likelihood = likelihood


class GPR(object):
    def __init__(self, latent=None, lr=.01, max_iterations=200, kernel_params=None, latent_params=None,
                 learn_likelihood_noise=True, dtype=np.float64, device=0, fit_method='adam', fixed_effects=None,
                 fit_objective='mll'):
        if fit_method not in ('adam', 'ai'):
            raise ValueError("fit_method is 'adam' or 'ai', got %r" % (fit_method,))
        if fit_objective not in ('mll', 'reml'):
            raise ValueError("fit_objective is 'mll' or 'reml', got %r" % (fit_objective,))
        if not (fixed_effects is None or fixed_effects in ('intercept', 'linear') or callable(fixed_effects)):
            raise ValueError("fixed_effects is None, 'intercept', 'linear' or a callable x -> (n, p), got %r" % (fixed_effects,))
        if fit_objective == 'reml' and fixed_effects is None:
            fixed_effects = 'intercept'                # REML of the constant mean: one degree of freedom
        self.fit_method = fit_method
        self.fixed_effects = fixed_effects
        self.fit_objective = fit_objective
        self.fit_info = None
        self._train_x = None
        self._train_y = None
        self._train_y_mean = None
        self._train_var = None
        self.likelihood = None
        self.model = None
        self.optimizer = None
        self.lr_scheduler = None
        self.lr = lr
        self.latent = latent
        self.kernel_params = kernel_params
        self.latent_params = latent_params
        self.max_iter = max_iterations
        self.learn_likelihood_noise = learn_likelihood_noise
        self.dtype = np.dtype(dtype)
        self.device = device
        self._ctx = None
        self._hyp_key = None

    # ---- device context -------------------------------------------------------------------
    @property
    def ctx(self):
        if self._ctx is None:
            self._ctx = _hip.Context(self.dtype, self.device)      # raises without a GPU: no fallback
        return self._ctx

    def hypers(self):
        """(log_lengthscale[D], log_outputscale, log_noise, kernel id) as plain floats.  Under the additive kernel the
        lengthscales of the two parts in coordinate order, log_outputscale a pair and the id ('additive', split, id_a, id_b)."""
        m = self.model
        if m.sep is not None:
            # the separable product: the lengthscales of the two parts in coordinate order, id ('separable', split, id_a, id_b);
            # with the genotype term (log os, log os_g) and ('genotype', ('separable', split, id_a, id_b))
            sk = m.kernel_covar_module if m.relationship is None else m.kernel_covar_module.kernels[0]
            ls = np.concatenate([k.log_lengthscale.detach().double().reshape(-1).numpy() for k in sk.base_kernel.kernels])
            los = float(sk.log_outputscale.item())
            if m.relationship is not None:
                los = (los, float(m.kernel_covar_module.kernels[1].log_outputscale.item()))
            return ls, los, float(self.likelihood.log_noise.item()), m.kernel_type
        if m.relationship is not None:         # D - 1 spatial lengthscales, (log os_a, log os_g), ('genotype', id_a)
            ks = m.kernel_covar_module.kernels
            return (ks[0].base_kernel.log_lengthscale.detach().double().reshape(-1).numpy().copy(),
                    (float(ks[0].log_outputscale.item()), float(ks[1].log_outputscale.item())),
                    float(self.likelihood.log_noise.item()), m.kernel_type)
        if m.split is not None:
            ks = m.kernel_covar_module.kernels
            ls = np.concatenate([k.base_kernel.log_lengthscale.detach().double().reshape(-1).numpy() for k in ks])
            return (ls, tuple(float(k.log_outputscale.item()) for k in ks), float(self.likelihood.log_noise.item()),
                    m.kernel_type)
        return (m.kernel_covar_module.base_kernel.log_lengthscale.detach().double().reshape(-1).numpy().copy(),
                float(m.kernel_covar_module.log_outputscale.item()), float(self.likelihood.log_noise.item()),
                m.kernel_type)

    def sync_hypers(self):
        """Push the current parameters to the device context if they changed."""
        ls, los, ln, kt = self.hypers()
        key = (tuple(ls), los, ln, kt)
        if key != self._hyp_key:
            self.push_hypers(self.ctx)
            self._hyp_key = key
            return True
        return False

    def push_hypers(self, ctx):
        """Set the current hyper-parameters on `ctx` (this model's own context, or another one that is to compute with them)."""
        ls, los, ln, kt = self.hypers()
        if isinstance(kt, tuple) and kt[0] == 'separable':
            ctx.set_hypers_separable(ls, kt[1], los, ln, kernel_a=kt[2], kernel_b=kt[3])
        elif isinstance(kt, tuple) and kt[0] == 'genotype' and isinstance(kt[1], tuple):
            G, Q = self.model.relationship
            ctx.set_hypers_separable(ls, kt[1][1], los[0], ln, kernel_a=kt[1][2], kernel_b=kt[1][3], log_outputscale_g=los[1], G=G,
                                     n_genotypes=Q)
        elif isinstance(kt, tuple) and kt[0] == 'genotype':
            G, Q = self.model.relationship
            ctx.set_hypers_relationship(ls, los[0], los[1], ln, kernel_a=kt[1], G=G, n_genotypes=Q)
        elif isinstance(kt, tuple):
            ctx.set_hypers_additive(ls, kt[1], los[0], los[1], ln, kt[2], kt[3])
        else:
            ctx.set_hypers(ls, los, ln, kt)

    # ---- models.py:103-115 ------------------------------------------------------------------
    @property
    def train_x(self):
        return self._train_x

    @property
    def train_y(self):
        return self._train_y

    @property
    def train_var(self):
        return self._train_var

    # ---- models.py:117-135 ------------------------------------------------------------------
    def reset(self, x, y, var):
        self.set_train_data(x, y, var)
        self.likelihood = _GaussianLikelihood()
        self.model = ExactGPModel(self._train_x, self._zero_mean_train_y, self.likelihood, self._train_var, self.latent,
                                  self.kernel_params, self.latent_params)
        params = [p for n, p in self.model.named_parameters()
                  if self.learn_likelihood_noise or n != 'likelihood.log_noise']
        self.optimizer = torch.optim.Adam([{'params': params}, ], lr=self.lr)
        self.lr_scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(self.optimizer, mode='min', patience=50)
        self._hyp_key = None

    def set_train_data(self, x, y, var=None):
        x = np.asarray(x, dtype=np.float64)
        self._train_x = x.reshape(len(x), -1)
        self._train_y = np.asarray(y, dtype=np.float64).reshape(-1)
        self._train_y_mean = float(np.mean(self._train_y)) if len(self._train_y) else 0.0     # models.py:129
        self._zero_mean_train_y = self._train_y - self._train_y_mean                         # models.py:130
        if var is not None:
            self._train_var = np.asarray(var, dtype=np.float64).reshape(-1)

    # ---- fixed effects ------------------------------------------------------------------------
    def fixed_basis(self, x, train_x=None):
        """The (n, p) basis h(x) of the fixed effects, or None without any: 'intercept' is the constant; 'linear' the constant
        and every coordinate centred on the train sites' mid-range and scaled by their range (train_x: the stored train
        inputs by default; the genotype id column is no coordinate); a callable is evaluated on x."""
        if self.fixed_effects is None:
            return None
        x = np.asarray(x, dtype=np.float64)
        x = x.reshape(len(x), -1)
        if callable(self.fixed_effects):
            H = np.asarray(self.fixed_effects(x), dtype=np.float64).reshape(len(x), -1)
        elif self.fixed_effects == 'intercept':
            H = np.ones((len(x), 1))
        else:
            ref = self._train_x if train_x is None else np.asarray(train_x, dtype=np.float64).reshape(len(train_x), -1)
            genotype = self.kernel_params is not None and self.kernel_params.get('type') == 'genotype'
            nc = x.shape[1] - 1 if genotype else x.shape[1]
            lo, hi = ref[:, :nc].min(0), ref[:, :nc].max(0)
            H = np.c_[np.ones(len(x)), (x[:, :nc] - 0.5 * (lo + hi)) / np.where(hi > lo, hi - lo, 1.0)]
        if not 1 <= H.shape[1] <= 16:
            raise ValueError('fixed_effects: 1 <= p <= 16 basis columns, got %d' % H.shape[1])
        return H

    def fixed_effect_estimates(self):
        """(beta, cov beta): the generalised-least-squares estimates of the fixed effects at the current hyper-parameters and
        their covariance (H' S^-1 H)^-1, from the stored training data (algp_get_gls)."""
        if self.fixed_effects is None:
            raise ValueError('fixed_effect_estimates needs fixed_effects')
        if self.model is None:
            raise ValueError('fixed_effect_estimates: fit or reset the model first')
        self._load_train_on_device()
        self.ctx.factorize()
        beta, cov, _ = self.ctx.gls(want_reml=False)
        return beta, cov

    # ---- models.py:137-159 ------------------------------------------------------------------
    def _load_train_on_device(self):
        c = self.ctx
        self.sync_hypers()
        c.set_pool(self._train_x)
        if self.fixed_effects is not None:
            c.set_fixed_effects(self.fixed_basis(self._train_x))
        c.set_train(np.arange(len(self._train_x)), self._train_y, self._train_var)

    def _objective_step(self, want_value=True, want_grad=True):
        """One device step of the fit's objective: (MLL, gradient) or, with fit_objective='reml', (l_R, gradient)."""
        if self.fit_objective == 'reml':
            return self.ctx.reml_step(want_value, want_grad)
        return self.ctx.fit_step(want_value, want_grad)

    def _information(self):
        return self.ctx.reml_ai() if self.fit_objective == 'reml' else self.ctx.mll_ai()

    def neg_mll_and_grad(self):
        """loss = -MLL/N (-l_R/N with fit_objective='reml') and its gradient w.r.t. the model parameters, from the device."""
        c = self.ctx
        if self.sync_hypers():
            pass
        mll, grad = self._objective_step()   # factorisation + objective + gradient: one ABI call per Adam iteration
        n = max(1, len(self._train_y))
        return -mll / n, -grad / n

    def _gradient_route(self):
        """[(name, parameter, a, b)]: the parameter that entries [a, b) of the device's gradient (and of the average-information
        matrix's rows and columns) belong to, in the device's order."""
        named = dict(self.model.named_parameters())
        noise = 'likelihood.log_noise'
        if self.model.sep is not None and self.model.relationship is not None:
            # the D + 2 gradient: [log ls of part a, of part b | log os, log os_g | log noise]
            names = ['kernel_covar_module.kernels.0.base_kernel.kernels.%d.log_lengthscale' % k for k in (0, 1)] + \
                    ['kernel_covar_module.kernels.0.log_outputscale', 'kernel_covar_module.kernels.1.log_outputscale', noise]
        elif self.model.sep is not None:
            # the D + 2 gradient: [log ls of part a, of part b | log os | log noise]
            names = ['kernel_covar_module.base_kernel.kernels.%d.log_lengthscale' % k for k in (0, 1)] + \
                    ['kernel_covar_module.log_outputscale', noise]
        elif self.model.relationship is not None:
            # the D + 2 gradient: [log ls of the D - 1 spatial coordinates | log os_a, log os_g | log noise]
            names = ['kernel_covar_module.kernels.0.base_kernel.log_lengthscale', 'kernel_covar_module.kernels.0.log_outputscale',
                     'kernel_covar_module.kernels.1.log_outputscale', noise]
        elif self.model.split is not None:
            # the D + 3 gradient: [log ls in coordinate order | log os_a, log os_b | log noise]
            names = ['kernel_covar_module.kernels.%d.base_kernel.log_lengthscale' % k for k in (0, 1)] + \
                    ['kernel_covar_module.kernels.%d.log_outputscale' % k for k in (0, 1)] + [noise]
        else:
            names = ['kernel_covar_module.base_kernel.log_lengthscale', 'kernel_covar_module.log_outputscale', noise]
        route, at = [], 0
        for name in names:
            p = named[name]
            route.append((name, p, at, at + p.numel()))
            at += p.numel()
        return route

    def _scalar_names(self, route):
        """One name per scalar of the gradient: the parameter's, with [d] behind it where it has more than one entry."""
        return [name if b - a == 1 else '%s[%d]' % (name, d) for name, _, a, b in route for d in range(b - a)]

    def _learned(self, route):
        """The gradient's entries that fit optimises: all, or all but the noise (the last one)."""
        P = route[-1][3]
        return np.arange(P if self.learn_likelihood_noise else P - 1)

    def _fit_ai(self, disp=False):
        """fit by utils.ai_newton: damped Newton steps on the average-information matrix from the model's current parameters,
        one algp_fit_step per evaluation and one algp_get_mll_ai per accepted point; max_iterations caps the evaluations."""
        from .utils import ai_newton
        route = self._gradient_route()
        c = self.ctx
        n = max(1, len(self._train_y))
        self.fit_info = None
        if self.max_iter <= 0:
            return []

        def push(theta):
            with torch.no_grad():
                for _, p, a, b in route:
                    p.copy_(torch.from_numpy(np.array(theta[a:b], dtype=np.float64)).reshape(p.shape))
            self.sync_hypers()

        def value_and_grad(theta):
            push(theta)
            mll, g = self._objective_step()  # raises LinAlgError (ALGP_ERR_NOT_PD) where S has no factor: a rejected trial
            if disp:
                print(-mll / n)
            return mll, g

        theta0 = np.concatenate([p.detach().double().reshape(-1).numpy() for _, p, _, _ in route])
        theta, info = ai_newton(theta0, value_and_grad, lambda theta: self._information(), free=self._learned(route),
                                max_evaluations=self.max_iter, n=n)
        push(theta)                          # (the last trial may have been a rejected one)
        info['objective'] = self.fit_objective
        self.fit_info = info
        losses = [-m / n for m in info['trace']]
        print('Initial LogLikelihood {:.3f} Final LogLikelihood {:.3f}'.format(-losses[0], -losses[-1]))
        return losses

    def hyper_covariance(self):
        """(names, cov): the inverse of the average-information matrix of the MLL (algp_get_mll_ai) restricted to the learned
        parameters, at the current hyper-parameters and train data -- one fit step and one AI matrix on the device, after
        either fit method.  names: the named_parameters names in the gradient's order, one per scalar ('...[d]' for entry d of
        a lengthscale vector).  The parameters are the LOG lengthscales, outputscales and noise.  This is the asymptotic
        covariance of the estimates only at a stationary point of the MLL (a converged fit: fit_info['reason'] == 'gradient');
        anywhere else it is just the inverse curvature there."""
        if self.model is None:
            raise ValueError('hyper_covariance: fit or reset the model first')
        route = self._gradient_route()
        self._load_train_on_device()
        self._objective_step(want_grad=False)
        ai = self._information()             # the restricted likelihood's with fit_objective='reml'
        keep = self._learned(route)
        names = self._scalar_names(route)
        return [names[k] for k in keep], np.linalg.inv(ai[np.ix_(keep, keep)])

    def hyper_standard_errors(self):
        """{name: standard error} of the learned log hyper-parameters: the square roots of hyper_covariance()'s diagonal (and
        with its caveat: at a stationary point only)."""
        names, cov = self.hyper_covariance()
        return dict(zip(names, np.sqrt(np.diag(cov))))

    def heritability(self):
        """(h2, se) under the genotype kernel: h2 = gbar os_g / (gbar os_g + os_a + sigma_n^2) with gbar the mean diagonal of
        the relationship matrix, and its delta-method standard error from hyper_covariance() (utils.heritability)."""
        if self.model is None or self.model.relationship is None:
            raise ValueError("heritability needs kernel_params['type'] = 'genotype'")
        from .utils import heritability
        G, _ = self.model.relationship
        names, cov = self.hyper_covariance()
        _, los, ln, _ = self.hypers()
        at = [names.index('kernel_covar_module.kernels.0.log_outputscale'), names.index('kernel_covar_module.kernels.1.log_outputscale')]
        if self.learn_likelihood_noise:
            at.append(names.index('likelihood.log_noise'))
        return heritability(los[0], los[1], ln, 1.0 if G is None else float(np.mean(np.diag(G))), cov[np.ix_(at, at)])

    def ar1_correlations(self, spacing=1.0):
        """[(rho, se), (rho, se)] of the two parts of the separable kernel where each is Matern-1/2 over a single coordinate -- an
        AR1 process along that coordinate: rho = exp(-spacing / ls) is the correlation of two sites `spacing` apart (one plot
        for coordinates counted in plots), and se = rho (spacing / ls) se(log ls) its delta-method standard error from
        hyper_covariance() (with that method's caveat: at a stationary point only).  ValueError for any other kernel or part."""
        if self.model is None or self.model.sep is None:
            raise ValueError("ar1_correlations needs the separable kernel (kernel_params['type'] = 'separable', or the genotype "
                             "kernel's 'spatial' entry)")
        split, ids = self.model.sep[0], self.model.sep[1:]
        ls = np.exp(self.hypers()[0])
        widths = (split, len(ls) - split)
        for k in (0, 1):
            if ids[k] != _hip.KERNEL_MATERN05 or widths[k] != 1:
                raise ValueError('ar1_correlations: part %d is not Matern-1/2 over a single coordinate (kernel id %d over %d '
                                 'coordinate(s))' % (k, ids[k], widths[k]))
        names, cov = self.hyper_covariance()
        head = 'kernel_covar_module.' if self.model.relationship is None else 'kernel_covar_module.kernels.0.'
        out = []
        for k in (0, 1):
            at = names.index(head + 'base_kernel.kernels.%d.log_lengthscale' % k)
            rho = float(np.exp(-spacing / ls[k]))
            out.append((rho, float(rho * (spacing / ls[k]) * np.sqrt(max(cov[at, at], 0.0)))))
        return out

    def fit(self, x, y, var=None, disp=False):
        if var is None:
            var = np.full(len(y), 1e-5)                                           # models.py:138-139
        self.reset(x, y, var)
        self._load_train_on_device()
        if self.fit_method == 'ai':
            return self._fit_ai(disp)
        named = dict(self.model.named_parameters())
        p_n = named['likelihood.log_noise']
        if self.model.relationship is not None or self.model.split is not None or self.model.sep is not None:
            route = [(p, a, b) for _, p, a, b in self._gradient_route()]
        else:
            p_ls = named['kernel_covar_module.base_kernel.log_lengthscale']
            p_os = named['kernel_covar_module.log_outputscale']
            D = p_ls.numel()
            route = None
        initial_ll = final_ll = None
        losses = []
        for i in range(self.max_iter):
            self.optimizer.zero_grad()
            loss, g = self.neg_mll_and_grad()
            if route is not None:
                for p, a, b in route:
                    p.grad = torch.from_numpy(g[a:b].copy()).reshape(p.shape)
            else:
                p_ls.grad = torch.from_numpy(g[:D].copy()).reshape(p_ls.shape)
                p_os.grad = torch.tensor([g[D]], dtype=torch.float64)
                p_n.grad = torch.tensor([g[D + 1]], dtype=torch.float64)
            self.optimizer.step()
            self.lr_scheduler.step(loss)
            if disp:
                print(i, loss)
            if i == 0:
                initial_ll = -loss
            final_ll = -loss
            losses.append(loss)
        if self.max_iter > 0:
            print('Initial LogLikelihood {:.3f} Final LogLikelihood {:.3f}'.format(initial_ll, final_ll))
        self.sync_hypers()
        if self.fit_objective == 'reml':
            self.fit_info = {'objective': 'reml', 'evaluations': len(losses)}
        return losses

    # ---- models.py:161-181 ------------------------------------------------------------------
    def cov_mat(self, x1, x2=None, white_noise_var=None, add_likelihood_var=False):
        self.sync_hypers()
        x1 = np.asarray(x1, dtype=self.dtype)
        x1 = x1.reshape(len(x1), -1)
        if x2 is not None:
            x2 = np.asarray(x2, dtype=self.dtype)
            x2 = x2.reshape(len(x2), -1)
            if x2.shape == x1.shape and np.array_equal(x1, x2):                   # models.py:169 torch.equal
                x2 = None
        if x2 is None:
            return self.ctx.kernel_matrix(x1, None, white_noise_var, add_likelihood_var)
        cov = self.ctx.kernel_matrix(x1, x2)
        if white_noise_var is not None:                                          # models.py:175-176 (square only)
            cov += np.diag(np.asarray(white_noise_var, dtype=self.dtype))
        if add_likelihood_var:
            cov += self.dtype.type(np.exp(self.likelihood.log_noise.item())) * np.eye(len(cov), dtype=self.dtype)
        return cov

    # ---- models.py:183-197 ------------------------------------------------------------------
    def predict(self, x, return_cov=False, return_std=False):
        """Posterior of the noisy observation y* = f* + eps (the likelihood is applied, as
        models.py:191 does), conditioned on the stored training data."""
        c = self.ctx
        self.sync_hypers()
        x = np.asarray(x, dtype=np.float64)
        x = x.reshape(len(x), -1)
        N, M = len(self._train_x), len(x)
        c.set_pool(np.vstack([self._train_x, x]))
        if self.fixed_effects is not None:
            c.set_fixed_effects(self.fixed_basis(np.vstack([self._train_x, x])))
        c.set_train(np.arange(N), self._train_y, self._train_var)
        noise = float(np.exp(self.likelihood.log_noise.item()))
        if self.fixed_effects is not None:
            # the trend-aware mean, and the variance with the universal-kriging term (algp_get_posterior_fixed)
            c.set_candidates(np.arange(N, N + M), prior_includes_noise=False)
            c.fit_and_solve()
            mu, var, proj = c.posterior_fixed(want_var=return_std, want_proj=return_cov and not return_std)
            if return_std:
                return mu, var + self.dtype.type(noise)
            if not return_cov:
                return mu
            cov, _ = c.posterior_cov()
            return mu, cov + proj @ proj.T + self.dtype.type(noise) * np.eye(M, dtype=self.dtype)
        if not (return_std or return_cov):
            c.factorize()
            return c.posterior_mean(np.arange(N, N + M))
        c.set_candidates(np.arange(N, N + M), prior_includes_noise=False)
        c.fit_and_solve()                                                        # factorisation + V^T in one launch where it fits
        mu, var = c.posterior()
        if return_std:                                                           # models.py:193 returns the variance
            return mu, var + self.dtype.type(noise)
        cov, _ = c.posterior_cov()
        return mu, cov + self.dtype.type(noise) * np.eye(M, dtype=self.dtype)

    def predict_components(self, x):
        """(mean_a, mean_b): the two parts' shares of the posterior mean of the latent field at `x` under the additive kernel
        -- with the genotype coordinates first, mean_a is the genotype effect adjusted for spatial trend.  The constant mean
        belongs to neither: mean_a + mean_b + mean(train y) = predict(x).  With fixed effects the shares are taken with the
        effects estimated (alpha_R in alpha's place) and the trend's share is predict_trend's: mean_a + mean_b + predict_trend(x)
        + mean(train y) = predict(x)."""
        if self.model is None or (self.model.split is None and self.model.relationship is None):
            raise ValueError("predict_components needs kernel_params['type'] = 'additive' or 'genotype'")
        c = self.ctx
        idx = self._load_pool_with(x)
        if self.fixed_effects is not None:
            return c.posterior_mean_fixed(0, idx), c.posterior_mean_fixed(1, idx)
        return c.posterior_mean_component(0, idx), c.posterior_mean_component(1, idx)

    def predict_trend(self, x):
        """The fixed effects' share h(x)' beta of the posterior mean at `x`, beta estimated by generalised least squares at the
        current hyper-parameters (algp_posterior_mean_fixed, component 2)."""
        if self.fixed_effects is None:
            raise ValueError('predict_trend needs fixed_effects')
        if self.model is None:
            raise ValueError('predict_trend: fit or reset the model first')
        return self.ctx.posterior_mean_fixed(2, self._load_pool_with(x))

    def _load_pool_with(self, x):
        """Pool = train sites then `x` (the basis over both with fixed effects), train set, factorisation; x's pool indices."""
        c = self.ctx
        self.sync_hypers()
        x = np.asarray(x, dtype=np.float64)
        x = x.reshape(len(x), -1)
        N, M = len(self._train_x), len(x)
        c.set_pool(np.vstack([self._train_x, x]))
        if self.fixed_effects is not None:
            c.set_fixed_effects(self.fixed_basis(np.vstack([self._train_x, x])))
        c.set_train(np.arange(N), self._train_y, self._train_var)
        c.factorize()
        return np.arange(N, N + M)

    def genotype_effects(self, return_cov=False):
        """(mean, var), or (mean, cov) with return_cov: the posterior of the Q genotype effects under the genotype kernel,
        conditioned on the stored training data -- BLUPs, prediction-error variances or the joint covariance for rankings and
        contrasts, genotypes without a plot included (algp_genotype_posterior).  With fixed effects the BLUPs are adjusted for
        the estimated effects and the variances carry beta's uncertainty, as the mixed-model equations give them
        (algp_genotype_posterior_fixed)."""
        if self.model is None or self.model.relationship is None:
            raise ValueError("genotype_effects needs kernel_params['type'] = 'genotype'")
        c = self.ctx
        self.sync_hypers()
        c.set_pool(self._train_x)
        if self.fixed_effects is not None:
            c.set_fixed_effects(self.fixed_basis(self._train_x))
        c.set_train(np.arange(len(self._train_x)), self._train_y, self._train_var)
        c.factorize()
        if self.fixed_effects is not None:
            mean, var, cov = c.genotype_posterior(want_var=not return_cov, want_cov=return_cov, fixed=True)
            return (mean, cov) if return_cov else (mean, var)
        mean, var, cov = c.genotype_posterior(want_var=not return_cov, want_cov=return_cov)
        return (mean, cov) if return_cov else (mean, var)

    def sample_posterior(self, x, n_samples=1, n_features=2048, rng=None):
        """(n_samples, len(x)) joint draws of the latent field f at `x` (no observation noise), conditioned on the stored
        training data: utils.posterior_samples."""
        from .utils import posterior_samples
        return posterior_samples(self, self._train_x, self._train_y, x, self._train_var, n_samples=n_samples,
                                 n_features=n_features, rng=rng)

    def group_posterior(self, x, group, test_var=None, weight=None, n_groups=None, return_cross=False):
        """(mean, cov) or (mean, cov, cross) of the aggregates of the latent field f over groups of the sites `x`, conditioned
        on the stored training data: utils.group_posterior.  With fixed effects: of the total signal with the effects estimated."""
        from .utils import group_posterior
        return group_posterior(self, self._train_x, self._train_y, x, group, self._train_var, test_var=test_var, weight=weight,
                               n_groups=n_groups, return_cross=return_cross)

    def get_embeddings(self, x):
        return np.asarray(x)                                                     # identity latent (models.py:199-203)
