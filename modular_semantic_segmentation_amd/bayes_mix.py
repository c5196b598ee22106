"""Bayes fusion of the experts' label maps (reference: xview/models/bayes_mix.py)."""
from itertools import product

import numpy as np
import torch

from . import ops
from .base_model import grouped_batches
from .basic_fusion_model import (FusionModel, device_tables, fused_head_applicable, grid_point_configs, grid_results,
                                 multi_head_applicable, reduce_over_ranks, run_lowres_scores, score_grid_fused,
                                 score_grid_fused_multi, score_grid_generic)

UNIFORM_PRIOR = 1.0 / 14     # the reference hard-codes 1/14 regardless of num_classes (bayes_mix.py:42,95)


def _conditional(confusion_T):
    """p(expert output | ground-truth class): nan_to_num(M / M.sum(0)) (bayes_mix.py:36,86)."""
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.nan_to_num(confusion_T / confusion_T.sum(0))


def _prior(confusion_T_last, class_prior):
    """bayes_mix.py:42-54: the data prior comes from the LAST expert's matrix."""
    data_prior = confusion_T_last.sum(0) / confusion_T_last.sum()
    if class_prior == 'uniform':
        return UNIFORM_PRIOR
    if class_prior == 'data':
        return data_prior
    weight = float(class_prior)
    prior = weight * UNIFORM_PRIOR + (1 - weight) * data_prior
    return prior / prior.sum()


def bayes_tables(confusion_matrices, class_prior='data'):
    """Host precompute for xv_bayes_fuse: float32 loglik [E,C,C] = log(1e-20 + cond_e) and
    logprior [C] = log(prior), the per-class constants of bayes_fusion (bayes_mix.py:33-58).
    confusion_matrices: list of float32 [C,C] already transposed (rows = predicted)."""
    C = confusion_matrices[0].shape[0]
    loglik = np.stack([np.log(np.float32(1e-20) + _conditional(m).astype(np.float32), dtype=np.float32)
                       for m in confusion_matrices])
    prior = np.broadcast_to(np.asarray(_prior(confusion_matrices[-1], class_prior), np.float32), (C,))
    with np.errstate(divide='ignore'):
        logprior = np.log(prior, dtype=np.float32)
    return np.ascontiguousarray(loglik), np.ascontiguousarray(logprior)


def bayes_fusion(classifications, confusion_matrices, class_prior='data'):
    """Functional entry point with the reference's signature (bayes_mix.py:12-58;
    experiments/timing.py:52-80).  classifications: list of int64 CUDA tensors [N,H,W].
    Returns (score f32 [N,H,W,C], log_likelihoods, conditionals); the per-expert lists hold the
    [C,C] tables the per-pixel gathers of the reference index into."""
    loglik, logprior = bayes_tables(confusion_matrices, class_prior)
    _, score = ops.bayes_fuse(list(classifications), *device_tables(classifications[0].device, loglik, logprior),
                              want_score=True)
    return score, [l for l in loglik], [_conditional(m) for m in confusion_matrices]


def bayes_decision_matrix(confusion_matrices, class_prior='data'):
    """Lookup table of the fused class for every combination of expert outputs
    (bayes_mix.py:61-112); float64 host math, int64 [C]*E."""
    num_classes = confusion_matrices[0].shape[0]
    num_experts = len(confusion_matrices)
    combos = np.array(list(product(*(range(num_classes) for _ in range(num_experts)))))
    log_likelihoods = np.zeros((combos.shape[0], num_experts, num_classes))
    for e, m in enumerate(confusion_matrices):
        with np.errstate(divide='ignore'):
            log_likelihoods[:, e, :] = np.log(1e-20 + _conditional(m)[combos[:, e]])
    with np.errstate(divide='ignore'):
        fused = np.argmax(log_likelihoods.sum(1) + np.log(_prior(confusion_matrices[-1], class_prior)), axis=1)
    return fused.reshape([num_classes for _ in range(num_experts)])


def fused_decision_table(loglik, logprior):
    """dec[a][b] = argmax_k ((loglik[0][a][k] + loglik[1][b][k]) + logprior[k]), lowest index on ties: the table the fused
    Bayes head builds in LDS from float32 tables, with its float32 sums in its order (bayes_decision_matrix is the float64
    form of the decision_matrix=True path; the two may differ where two classes tie within float32)."""
    loglik, logprior = np.asarray(loglik, np.float32), np.asarray(logprior, np.float32)
    with np.errstate(invalid='ignore'):
        total = (loglik[0][:, None, :] + loglik[1][None, :, :]) + logprior
    return np.argmax(total, axis=-1)


def confusion_from_joint_hist(hist, decision):
    """cm[l][decision[a][b]] += hist[l][a][b]: the confusion matrix of a fusion that decides by the experts' label pair."""
    C = hist.shape[0]
    cm = np.zeros((C, C), hist.dtype)
    for k in range(C):
        cm[:, k] = hist[:, decision == k].sum(-1)
    return cm


class BayesFusion(FusionModel):
    """config: num_units, num_classes (via data_description), prefixes, num_channels, expert_model,
    class_prior ('data' | 'uniform' | float), confusion_matrices {modality: [C,C] label x pred};
    decision_matrix=True fuses two experts through the bayes_decision_matrix lookup table instead of the
    per-pixel log-likelihood sum (the faster variant timed by experiments/timing.py:87-115); fused_head=False keeps
    the experts' label maps materialised (`expert_outputs`) instead of fusing inside the decoder-head kernel."""

    def __init__(self, output_dir=None, confusion_matrices=False, **config):
        standard_config = {'learning_rate': 0.0, 'class_prior': 'data'}
        standard_config.update(config)
        self.confusion_matrices = {}
        if not confusion_matrices:
            raise UserWarning('ERROR: BayesFusion needs confusion_matrices (the experiment database of '
                              'the reference, `eval_experiments`, is out of scope)')
        order = []
        for key, matrix in confusion_matrices.items():
            order.append(key)
            self.confusion_matrices[key] = np.asarray(matrix).astype('float32').T   # bayes_mix.py:141
        self._matrix_order = order
        FusionModel.__init__(self, 'BayesFusion', output_dir=output_dir, **standard_config)

    def _build_graph(self):
        FusionModel._build_graph(self)
        # modality order = order of the confusion_matrices dict (bayes_mix.py:137-141 overwrites
        # self.modalities before FusionModel.__init__ resets it from `prefixes`)
        mats = [self.confusion_matrices[m] for m in self.modalities]
        self.loglik, self.logprior = device_tables(self.device, *bayes_tables(mats, self.config['class_prior']))
        self.conditionals = [_conditional(m) for m in mats]
        lut = bayes_decision_matrix(mats, self.config['class_prior']).astype(np.int64)
        self.decision_matrix = device_tables(self.device, lut)[0]

    def _fused_head(self):
        if self.config.get('decision_matrix', False):
            return None             # the lookup table takes the experts' materialised label maps
        return lambda *scores: ops.fused_head(*scores, self.config['num_classes'], self.loglik, self.logprior)

    def _multi_head(self):
        if self.config.get('decision_matrix', False):
            return None             # as _fused_head: that configuration fuses the experts' materialised label maps
        return lambda *scores: ops.fused_head_multi(*scores, self.config['num_classes'], 'bayes', tab=self.loglik,
                                                    logprior=self.logprior)

    has_fused_score = True

    def _agreement_head(self):
        if self.config.get('decision_matrix', False):
            return None             # as _fused_head: the lookup table decides in float64, the head in float32
        return 'bayes', dict(tab=self.loglik, logprior=self.logprior)

    def _calibration_refusal(self):
        if self.config.get('decision_matrix', False):
            return 'decision_matrix=True fuses by a lookup table, which has no class scores to take a confidence from'
        return FusionModel._calibration_refusal(self)

    def _fusion(self, expert_outputs, output_attr=None):
        labels = [expert_outputs[m]['classification'] for m in self.modalities]
        want_score = output_attr == 'fused_score'
        if self.config.get('decision_matrix', False) and len(labels) == 2 and not want_score:
            self.probs = {m: expert_outputs[m].get('prob') for m in self.modalities}
            return ops.bayes_fuse_lut(labels[0], labels[1], self.decision_matrix)
        fused, score = ops.bayes_fuse(labels, self.loglik, self.logprior, want_score=want_score)
        self.probs = {m: expert_outputs[m].get('prob') for m in self.modalities}
        if want_score:
            return score
        if output_attr == 'probs':
            return torch.stack([self.probs[m] for m in self.modalities], 1)
        return fused

    # ---- grid search over the class prior on one pass of the experts ------------------------------------
    searchable = ('class_prior',)
    JOINT_HIST_MAX_CLASSES = 20         # xv_fused_head_joint_hist_fwd: C^3 u32 counters in one workgroup's LDS

    def score_grid(self, data, search_parameters, max_iterations=None):
        """score() under every `class_prior` of `search_parameters` on ONE pass of the experts over `data`: [(point config,
        measures, confusion matrix)] in parameter_combinations order, each pair what score() of a model with that config
        returns.  A Bayes-fused label is a function of the experts' label pair, so where the fused head serves the model the
        pass only counts the joint histogram of (ground truth, label a, label b) and every prior's matrix follows on the host."""
        configs = grid_point_configs(self, search_parameters, self.searchable)
        mats = [self.confusion_matrices[m] for m in self.modalities]
        C = self.config['num_classes']
        lut = self.config.get('decision_matrix', False)
        if not lut and fused_head_applicable(self) and C <= self.JOINT_HIST_MAX_CLASSES:
            hist = torch.zeros((C, C, C), dtype=torch.int64, device=self.device)

            def count_batch(Sa, Sb, ba, bb, n, hi, wi, labels, hist):
                ops.fused_head_joint_hist(Sa, Sb, ba, bb, n, hi, wi, C, labels, hist=hist)
            score_grid_fused(self, data, hist, count_batch, max_iterations)
            reduce_over_ranks(self, hist)
            hist = hist.cpu().numpy()
            counts = [confusion_from_joint_hist(hist, fused_decision_table(*bayes_tables(mats, c['class_prior'])))
                      for c in configs]
            return grid_results(configs, counts)
        if not lut and multi_head_applicable(self):
            # three or four experts: the log-likelihoods come from the matrices alone, a prior only changes logprior
            logprior = torch.stack([device_tables(self.device, bayes_tables(mats, c['class_prior'])[1])[0] for c in configs])
            counts = score_grid_fused_multi(self, data, 'bayes', len(configs), max_iterations, tab=self.loglik,
                                            logprior=logprior.contiguous())
            reduce_over_ranks(self, counts)
            return grid_results(configs, counts.cpu().numpy())
        if lut and len(self.modalities) == 2:
            luts = device_tables(self.device, *[bayes_decision_matrix(mats, c['class_prior']).astype(np.int64) for c in configs])

            def fuse_point(outs, g):
                return ops.bayes_fuse_lut(*[outs[m]['classification'] for m in self.modalities], luts[g])
        else:
            tables = [device_tables(self.device, *bayes_tables(mats, c['class_prior'])) for c in configs]

            def fuse_point(outs, g):
                return ops.bayes_fuse([outs[m]['classification'] for m in self.modalities], *tables[g])[0]
        counts = score_grid_generic(self, data, len(configs), ('classification',), fuse_point, max_iterations)
        reduce_over_ranks(self, counts)
        return grid_results(configs, counts.cpu().numpy())

    # ---- a confusion matrix per group of images on one pass (BaseModel.score_groups) ----------------------
    def _count_groups(self, data, ids, num_groups, max_iterations, scored):
        """Where the fused head serves the model the trunks stop at their low-resolution class scores and the pass counts the
        joint histogram per group; every group's matrix follows from it on the host as score_grid derives a prior's."""
        C = self.config['num_classes']
        if self.config.get('decision_matrix', False) or not fused_head_applicable(self) or C > self.JOINT_HIST_MAX_CLASSES:
            return FusionModel._count_groups(self, data, ids, num_groups, max_iterations, scored)
        hist = torch.zeros((num_groups, C, C, C), dtype=torch.int64, device=self.device)
        for batch, labels, batch_ids in grouped_batches(self, data, ids, num_groups, max_iterations, scored):
            Sa, Sb, ba, bb, n, hi, wi = run_lowres_scores(self, batch)
            ops.fused_head_joint_hist_grouped(Sa, Sb, ba, bb, n, hi, wi, C, labels, batch_ids, num_groups, hist=hist)
        reduce_over_ranks(self, hist)
        mats = [self.confusion_matrices[m] for m in self.modalities]
        decision = fused_decision_table(*bayes_tables(mats, self.config['class_prior']))
        return np.stack([confusion_from_joint_hist(h, decision) for h in hist.cpu().numpy()])
