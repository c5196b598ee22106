"""Dirichlet fusion of the experts' softmax outputs (reference: xview/models/dirichlet_mix.py)."""
from copy import deepcopy

import numpy as np
import torch
from scipy.special import gammaln

from . import ops
from .basic_fusion_model import (FusionModel, calibrate_experts, device_tables, engine_options, expert_factory,  # noqa: F401
                                 fused_head_applicable, grid_point_configs, grid_results, measure_experts,
                                 multi_head_applicable, reduce_over_ranks, run_experts, score_grid_fused,
                                 score_grid_fused_multi, score_grid_generic, test_pipeline)
from .dirichlet_fit import find_dirichlet_priors

UNIFORM_PRIOR = 1.0 / 14     # dirichlet_mix.py:116


def class_prior_vector(class_counts, class_prior, num_classes):
    """dirichlet_mix.py:115-129 (float32 like the graph constants)."""
    class_counts = np.asarray(class_counts, np.float32)
    data_prior = (class_counts / (1e-20 + class_counts.sum())).astype('float32')
    if class_prior == 'uniform':
        prior = UNIFORM_PRIOR
    elif class_prior == 'data':
        prior = data_prior
    else:
        weight = float(class_prior)
        prior = weight * UNIFORM_PRIOR + (1 - weight) * data_prior
        prior = prior / prior.sum()
    return np.broadcast_to(np.asarray(prior, np.float32), (num_classes,)).copy()


def dirichlet_tables(dirichlet_params, class_counts, class_prior, sigma):
    """Host precompute for xv_dirichlet_fuse from params[k, c] per expert:
    am1[e,c,k] = sigma*A_e[k,c] - 1, lognorm[e,c] = sum_k lgamma(sigma*A_e[k,c]) - lgamma(sum_k ..)
    ([TF1] Dirichlet.log_prob normaliser), logprior[c] = log(1e-20 + prior[c])  (dirichlet_mix.py:36)."""
    am1, lognorm = [], []
    for A in dirichlet_params:
        conc = (np.float32(sigma) * np.asarray(A, np.float32)).astype(np.float32)     # [k, c]
        am1.append((conc - np.float32(1)).T)
        c64 = conc.astype(np.float64)
        lognorm.append((gammaln(c64).sum(0) - gammaln(c64.sum(0))).astype(np.float32))
    C = am1[0].shape[0]
    prior = class_prior_vector(class_counts, class_prior, C)
    logprior = np.log(np.float32(1e-20) + prior, dtype=np.float32)
    return (np.ascontiguousarray(np.stack(am1), np.float32), np.ascontiguousarray(np.stack(lognorm), np.float32),
            np.ascontiguousarray(logprior, np.float32))


def dirichlet_fusion(probs, dirichlet_params, prior, sigma=1.0):
    """Functional entry point (dirichlet_mix.py:14-36; experiments/timing.py): probs = list of
    float32 CUDA tensors [N,H,W,C] (renormalised inside the kernel), dirichlet_params = list of
    [C,C] arrays (params[k, c]), prior = [C] probabilities.  Returns the fused score [N,H,W,C]."""
    am1, lognorm, _ = dirichlet_tables(dirichlet_params, np.ones(len(prior)), 'uniform', sigma)
    logprior = np.log(np.float32(1e-20) + np.asarray(prior, np.float32), dtype=np.float32)
    _, score = ops.dirichlet_fuse(list(probs), *device_tables(probs[0].device, am1, lognorm, logprior), want_score=True)
    return score


def fit_dirichlet_params(counts, class_counts, delta, beta, num_classes, modalities):
    """dirichlet_mix.py:207-257: {modality: [C,C] parameters} fitted on the host to the sufficient statistics `counts`
    {modality: [C,C]} and the class counts [C] under one (delta, beta) -- the fit of DirichletFusion and FusionComparison."""
    C = num_classes

    def dirichlet_em(measurements):
        params = np.ones((C, C)).astype('float64')
        for c in range(C):
            if class_counts[c] == 0:
                params[:, c] = np.ones(C)
                continue
            ss = (measurements[c, :] / class_counts[c]).astype('float64')
            neg_ss = (measurements.sum(0) - measurements[c, :]) / (class_counts.sum() - class_counts[c])
            params[:, c] = find_dirichlet_priors(ss, neg_ss, np.ones(C, 'float64'), max_iter=10000,
                                                 delta=delta, beta=beta)
        return params

    return {m: dirichlet_em(counts[m]) for m in modalities}


class DirichletFusion(FusionModel):
    """config: modalities, num_channels, num_units, expert_model, class_prior, sigma, delta, beta,
    optional dirichlet_params {modality: [C,C], 'class_counts': [C]}; the expert of modality m uses
    prefix m (dirichlet_mix.py:98)."""

    expert_wants = ('prob',)

    def __init__(self, output_dir=None, **config):
        standard_config = {'learning_rate': 0.0}
        standard_config.update(config)
        if 'dirichlet_params' in config:
            measurements = config['dirichlet_params']
            self.dirichlet_params = {m: np.asarray(measurements[m]).astype('float32') for m in config['modalities']}
            self.class_counts = np.asarray(measurements['class_counts']).astype('float32')
        else:
            print('WARNING: Could not yet import measurements, you need to fit this model first.')
        FusionModel.__init__(self, name='DirichletFusion', output_dir=output_dir, **standard_config)

    def _build_graph(self):
        FusionModel._build_graph(self)
        if hasattr(self, 'dirichlet_params'):
            self.am1, self.lognorm, self.logprior = device_tables(self.device, *dirichlet_tables(
                [self.dirichlet_params[m] for m in self.modalities], self.class_counts, self.config['class_prior'],
                self.config['sigma']))
        else:
            self.prediction = 0      # dirichlet_mix.py:165-168: no fusion possible before fit()

    def _predict_batch_impl(self, batch, output_attr=None):
        if not hasattr(self, 'am1'):
            raise UserWarning('ERROR: DirichletFusion has no measurements yet, call fit() first')
        self.probs = None       # (stays so on the fused route: the probabilities never leave the head's registers)
        return FusionModel._predict_batch_impl(self, batch, output_attr)

    def _fused_head(self):
        return lambda *scores: ops.fused_head(*scores, self.config['num_classes'], self.am1, self.logprior, lognorm=self.lognorm)

    def _multi_head(self):
        return lambda *scores: ops.fused_head_multi(*scores, self.config['num_classes'], 'dirichlet', tab=self.am1,
                                                    lognorm=self.lognorm, logprior=self.logprior)

    has_fused_score = True

    def _agreement_head(self):
        return 'dirichlet', dict(tab=self.am1, lognorm=self.lognorm, logprior=self.logprior)

    def _count_agreement(self, *args, **kwargs):
        if not hasattr(self, 'am1'):
            raise UserWarning('ERROR: DirichletFusion has no measurements yet, call fit() first')
        return FusionModel._count_agreement(self, *args, **kwargs)

    def _calibrate_batch(self, *args, **kwargs):
        if not hasattr(self, 'am1'):
            raise UserWarning('ERROR: DirichletFusion has no measurements yet, call fit() first')
        return FusionModel._calibrate_batch(self, *args, **kwargs)

    def _confidence_batch(self, *args, **kwargs):
        if not hasattr(self, 'am1'):
            raise UserWarning('ERROR: DirichletFusion has no measurements yet, call fit() first')
        return FusionModel._confidence_batch(self, *args, **kwargs)

    def _prediction_difference_batch(self, batch):
        if not hasattr(self, 'am1'):
            raise UserWarning('ERROR: DirichletFusion has no measurements yet, call fit() first')
        return FusionModel._prediction_difference_batch(self, batch)

    def _fusion(self, expert_outputs, output_attr=None):
        probs = [expert_outputs[m]['prob'] for m in self.modalities]
        self.probs = dict(zip(self.modalities, probs))
        want_score = output_attr == 'fused_score'
        fused, score = ops.dirichlet_fuse(probs, self.am1, self.lognorm, self.logprior, want_score=want_score)
        return score if want_score else fused

    # ---- fit = measure sufficient statistics on the GPU, Newton-fit on the host -------------------
    def _get_sufficient_statistic(self, data):
        """measure_experts over `data`, summed over the ranks (one process per GPU, each measured its shard of the data: one
        tiny all-reduce per tensor, RCCL over xGMI) whatever reduce_score_over_ranks says: ({modality: float64 [C,C]},
        int64 [C]) on the host."""
        from .parallel import allreduce_sum_
        S, counts, _ = measure_experts(self, data)
        allreduce_sum_(counts, *S.values())
        return {m: S[m].cpu().numpy() for m in S}, counts.cpu().numpy()

    def _fit_sufficient_statistic(self, counts, class_counts):
        """dirichlet_mix.py:207-257."""
        self.dirichlet_params = self._dirichlet_em(counts, class_counts, self.config['delta'], self.config['beta'])
        self.class_counts = class_counts
        self._initialize_graph()       # rebuild the tables with the new measurements

    def _dirichlet_em(self, counts, class_counts, delta, beta):
        """{modality: [C,C] parameters} fitted to the sufficient statistics under one (delta, beta)."""
        return fit_dirichlet_params(counts, class_counts, delta, beta, self.config['num_classes'], self.modalities)

    def fit(self, data, *args, **kwargs):
        """Measure the experts against the ground truth of `data`, then fit the class-conditional
        Dirichlets (dirichlet_mix.py:259-273).  Returns {modality: [C,C], 'class_counts': [C]}."""
        modality_counts, class_counts = self._get_sufficient_statistic(data)
        self.sufficient_statistics = (modality_counts, class_counts)      # what score_grid refits delta / beta from
        self._fit_sufficient_statistic(modality_counts, class_counts)
        ret = deepcopy(self.dirichlet_params)
        ret['class_counts'] = self.class_counts
        return ret

    # ---- grid search over the fusion parameters on one pass of the experts ------------------------------
    searchable = ('sigma', 'class_prior', 'delta', 'beta')

    def _grid_tables(self, configs):
        """Per grid point the (am1, lognorm, logprior) numpy tables dirichlet_tables gives a model of that config: sigma and
        class_prior only rebuild them; a (delta, beta) other than this model's re-runs the host fit, once per distinct pair,
        on the sufficient statistics of the last fit()."""
        own = (self.config.get('delta'), self.config.get('beta'))
        fitted = {}
        for config in configs:
            pair = (config.get('delta'), config.get('beta'))
            if pair in fitted:
                continue
            if pair == own and hasattr(self, 'dirichlet_params'):
                fitted[pair] = self.dirichlet_params
            elif not hasattr(self, 'sufficient_statistics'):
                raise UserWarning('ERROR: searching delta / beta needs the sufficient statistics of a fit(); call fit() first')
            else:
                fitted[pair] = self._dirichlet_em(*self.sufficient_statistics, delta=pair[0], beta=pair[1])
        return [dirichlet_tables([fitted[(c.get('delta'), c.get('beta'))][m] for m in self.modalities], self.class_counts,
                                 c['class_prior'], c['sigma']) for c in configs]

    def score_grid(self, data, search_parameters, max_iterations=None):
        """score() under every combination of `search_parameters` (lists of values for sigma, class_prior, delta, beta) on ONE
        pass of the experts over `data`: [(point config, measures, confusion matrix)] in parameter_combinations order, each
        pair what score() of a model with that config returns."""
        configs = grid_point_configs(self, search_parameters, self.searchable)
        if not hasattr(self, 'dirichlet_params') and not hasattr(self, 'sufficient_statistics'):
            raise UserWarning('ERROR: DirichletFusion has no measurements yet, call fit() first')
        tables = [device_tables(self.device, *point) for point in self._grid_tables(configs)]
        C = self.config['num_classes']
        if fused_head_applicable(self):
            am1, lognorm, logprior = (torch.stack([point[i] for point in tables]).contiguous() for i in range(3))
            counts = torch.zeros((len(configs), C, C), dtype=torch.int64, device=self.device)

            def count_batch(Sa, Sb, ba, bb, n, hi, wi, labels, cm):
                ops.fused_head_grid_score(Sa, Sb, ba, bb, n, hi, wi, C, am1, lognorm, logprior, labels, cm=cm)
            score_grid_fused(self, data, counts, count_batch, max_iterations)
        elif multi_head_applicable(self):
            am1, lognorm, logprior = (torch.stack([point[i] for point in tables]).contiguous() for i in range(3))
            counts = score_grid_fused_multi(self, data, 'dirichlet', len(configs), max_iterations, tab=am1, lognorm=lognorm,
                                            logprior=logprior)
        else:
            def fuse_point(outs, g):
                return ops.dirichlet_fuse([outs[m]['prob'] for m in self.modalities], *tables[g])[0]
            counts = score_grid_generic(self, data, len(configs), ('prob',), fuse_point, max_iterations)
        reduce_over_ranks(self, counts)
        return grid_results(configs, counts.cpu().numpy())
