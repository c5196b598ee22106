"""The reference's central comparison -- every expert alone, Bayes, Dirichlet and average fusion on one test split after
measuring the experts on the other -- on ONE pass of the experts per split (reference: experiments/bayes_fusion.py:146-195,
experiments/dirichlet_fusion.py:58-81, average_mix.py; there one model per row of the table).

The fusions differ only in what they do with the experts' outputs, so the trunks run once per batch.  Where the fused head
serves the model (two FCN experts with commuted heads) they stop at their 1/8-resolution class scores and three scoring heads
count from those: the joint histogram (both experts' matrices are its marginals, the Bayes matrix follows from the decision
table on the host), the grid-scoring head with one grid point (Dirichlet) and the counting form of the fused average head.
Otherwise -- any number of experts, AdapNet experts, fused_head=False, more classes than the joint histogram holds -- the
experts' labels and probabilities are materialised once and the stand-alone fusion kernels run on them.  Both routes count the
integers score() of the corresponding single model counts."""
from copy import deepcopy

import numpy as np
import torch

from . import ops
from .base_model import grouped_batches, grouped_results, groups_seen, image_groups, score_measures
from .basic_fusion_model import (FusionModel, _labelled_batches, device_tables, fused_head_applicable, measure_experts,
                                 multi_head_applicable, reduce_over_ranks, run_experts, run_lowres_scores,
                                 run_lowres_scores_multi)
from .bayes_mix import BayesFusion, bayes_tables, confusion_from_joint_hist, fused_decision_table
from .dirichlet_mix import dirichlet_tables, fit_dirichlet_params

FUSIONS = ('bayes_fusion', 'dirichlet_fusion', 'average_fusion')


def expert_matrices_from_joint_hist(hist):
    """The two experts' confusion matrices [C,C] (rows = ground truth) from hist[label][a][b]: its marginals."""
    hist = np.asarray(hist)
    return hist.sum(2), hist.sum(1)


class FusionComparison(FusionModel):
    """config: a Bayes-fusion configuration (prefixes, num_channels, num_units, expert_model, class_prior, ...) plus the
    Dirichlet fusion's sigma, delta, beta; optional measurements confusion_matrices {modality: [C,C] label x pred} and
    dirichlet_params {modality: [C,C], 'class_counts': [C]} -- what fit() measures and returns.  The Dirichlet fusion of the
    reference names an expert's variables by its modality: compare against a DirichletFusion with prefixes {m: m}."""

    def __init__(self, output_dir=None, confusion_matrices=None, dirichlet_params=None, **config):
        standard_config = {'learning_rate': 0.0, 'class_prior': 'data'}
        standard_config.update(config)
        for key in ('prior_strength', 'ibcc_max_iter', 'ibcc_tol'):
            if key in standard_config:
                raise NotImplementedError('FusionComparison has no IBCC row (config key %r): an IBCC fusion adapts to the data '
                                          'it scores, the rows here are frozen after fit(); score an IbccFusion itself' % key)
        for key in ('sigma', 'delta', 'beta'):
            if key not in standard_config:
                raise UserWarning('ERROR: FusionComparison needs %s (the Dirichlet fusion\'s parameter)' % key)
        self.confusion_matrices = None if not confusion_matrices else \
            {m: np.asarray(confusion_matrices[m]).astype(np.float64) for m in config['prefixes']}
        self.dirichlet_params = self.class_counts = None
        if dirichlet_params:
            self.dirichlet_params = {m: np.asarray(dirichlet_params[m]).astype('float32') for m in config['prefixes']}
            self.class_counts = np.asarray(dirichlet_params['class_counts']).astype('float32')
        FusionModel.__init__(self, 'FusionComparison', output_dir=output_dir, **standard_config)

    agreement_refusal = 'it scores several fusions and predicts with none: ask the fusion model itself'

    def _build_graph(self):
        FusionModel._build_graph(self)
        self._build_tables()

    def _build_tables(self):
        """The tables BayesFusion and DirichletFusion build from the same measurements and config."""
        self.bayes = self.dirichlet = None
        if self.confusion_matrices is not None:
            mats = [self.confusion_matrices[m].astype('float32').T for m in self.modalities]      # bayes_mix.py:141
            loglik, logprior = bayes_tables(mats, self.config['class_prior'])
            self.bayes = (loglik, logprior) + device_tables(self.device, loglik, logprior)
        if self.dirichlet_params is not None:
            self.dirichlet = device_tables(self.device, *dirichlet_tables(
                [self.dirichlet_params[m] for m in self.modalities], self.class_counts, self.config['class_prior'],
                self.config['sigma']))

    def _fusion(self, expert_outputs, output_attr=None):
        raise UserWarning('ERROR: FusionComparison scores several fusions, it predicts with none: use score_all(), or the '
                          'fusion model itself')

    # ---- measure both kinds of statistics on one pass ---------------------------------------------------
    def fit(self, measure_set, *args, **kwargs):
        """One pass of the experts over `measure_set`: every expert's confusion matrix (what BayesFusion is built from) and
        the Dirichlet sufficient statistics, then the host fit of DirichletFusion.  Returns {'confusion_matrices': {m: [C,C]},
        'dirichlet_params': {m: [C,C], 'class_counts': [C]}}."""
        C = self.config['num_classes']
        mods = self.modalities
        S, counts, cms = measure_experts(self, measure_set, confusion=True)
        reduce_over_ranks(self, *cms.values(), counts, *S.values())
        stats, class_counts = {m: S[m].cpu().numpy() for m in mods}, counts.cpu().numpy()
        self.sufficient_statistics = (stats, class_counts)
        self.confusion_matrices = {m: cms[m].cpu().numpy().astype(np.float64) for m in mods}
        self.dirichlet_params = fit_dirichlet_params(stats, class_counts, self.config['delta'], self.config['beta'], C, mods)
        self.class_counts = class_counts
        self._build_tables()
        params = deepcopy(self.dirichlet_params)
        params['class_counts'] = self.class_counts
        return {'confusion_matrices': deepcopy(self.confusion_matrices), 'dirichlet_params': params}

    # ---- score everything on one pass -------------------------------------------------------------------
    def one_pass_heads_applicable(self):
        """Two experts: the joint-histogram, grid-scoring and average counting heads (up to the joint histogram's class count);
        three or four: ops.fused_head_multi_count, which has no such limit."""
        return multi_head_applicable(self) or self._two_expert_heads_applicable()

    def _two_expert_heads_applicable(self):
        return fused_head_applicable(self) and self.config['num_classes'] <= BayesFusion.JOINT_HIST_MAX_CLASSES

    def _count_multi(self, head_args, labels, fused, experts, **groups):
        """Three or four experts, one batch: three counting launches on the same low-resolution scores -- Bayes (which also
        counts every expert's own matrix), Dirichlet with one point, mean -- into fused [3] and experts."""
        C = self.config['num_classes']
        am1, lognorm, logprior = self.dirichlet
        ops.fused_head_multi_count(*head_args, C, 'bayes', labels, tab=self.bayes[2], logprior=self.bayes[3][None].contiguous(),
                                   cm=fused[0], expert_cm=experts, **groups)
        ops.fused_head_multi_count(*head_args, C, 'dirichlet', labels, tab=am1[None].contiguous(),
                                   lognorm=lognorm[None].contiguous(), logprior=logprior[None].contiguous(), cm=fused[1], **groups)
        ops.fused_head_multi_count(*head_args, C, 'mean', labels, cm=fused[2], **groups)

    def _require_measurements(self):
        if self.bayes is None or self.dirichlet is None:
            raise UserWarning('ERROR: FusionComparison has no measurements yet, call fit() first')

    def _row_names(self):
        return list(self.modalities) + list(FUSIONS)

    def _rows(self, matrices):
        """{row name: (measures, confusion matrix float64)} from one matrix per row, each pair as score() returns it."""
        out = {}
        for name, cm in zip(self._row_names(), matrices):
            cm = np.asarray(cm).astype(np.float64)
            out[name] = (score_measures(cm), cm)
        return out

    def _generic_label_maps(self, batch):
        """The generic route of one batch: every expert once with labels and probabilities, then the stand-alone fusion
        kernels -> the five label maps, in row order."""
        am1, lognorm, logprior = self.dirichlet
        outs = run_experts(self, batch, ('classification', 'prob'))
        labs = [outs[m]['classification'].contiguous() for m in self.modalities]
        probs = [outs[m]['prob'] for m in self.modalities]
        fused = [ops.bayes_fuse(labs, self.bayes[2], self.bayes[3])[0], ops.dirichlet_fuse(probs, am1, lognorm, logprior)[0],
                 ops.average_fuse(probs)]
        return labs + [pred.contiguous() for pred in fused]

    def score_all(self, test_set, max_iterations=None):
        """One pass of the experts over `test_set`: {modality: (measures, confusion matrix), ..., 'bayes_fusion': ...,
        'dirichlet_fusion': ..., 'average_fusion': ...}, each pair what score() of the single model returns."""
        self._require_measurements()
        C = self.config['num_classes']
        am1, lognorm, logprior = self.dirichlet
        if multi_head_applicable(self):
            fused = torch.zeros((3, 1, C, C), dtype=torch.int64, device=self.device)       # Bayes, Dirichlet, average
            experts = torch.zeros((len(self.modalities), C, C), dtype=torch.int64, device=self.device)
            for batch, labels in _labelled_batches(self, test_set, max_iterations):
                self._count_multi(run_lowres_scores_multi(self, batch), labels, fused, experts)
            reduce_over_ranks(self, fused, experts)
            matrices = list(experts.cpu().numpy()) + list(fused[:, 0].cpu().numpy())
        elif self._two_expert_heads_applicable():
            hist = torch.zeros((C, C, C), dtype=torch.int64, device=self.device)
            counts = torch.zeros((2, C, C), dtype=torch.int64, device=self.device)         # Dirichlet, average
            tabs = (am1[None].contiguous(), lognorm[None].contiguous(), logprior[None].contiguous())
            for batch, labels in _labelled_batches(self, test_set, max_iterations):
                Sa, Sb, ba, bb, n, hi, wi = run_lowres_scores(self, batch)
                ops.fused_head_joint_hist(Sa, Sb, ba, bb, n, hi, wi, C, labels, hist=hist)
                ops.fused_head_grid_score(Sa, Sb, ba, bb, n, hi, wi, C, *tabs, labels, cm=counts[0:1])
                ops.fused_head_average_count(Sa, Sb, ba, bb, n, hi, wi, C, labels, cm=counts[1])
            reduce_over_ranks(self, hist, counts)
            hist, counts = hist.cpu().numpy(), counts.cpu().numpy()
            cm_a, cm_b = expert_matrices_from_joint_hist(hist)
            bayes = confusion_from_joint_hist(hist, fused_decision_table(self.bayes[0], self.bayes[1]))
            matrices = [cm_a, cm_b, bayes, counts[0], counts[1]]
        else:
            counts = torch.zeros((len(self._row_names()), C, C), dtype=torch.int64, device=self.device)
            for batch, labels in _labelled_batches(self, test_set, max_iterations):
                for i, pred in enumerate(self._generic_label_maps(batch)):
                    ops.confusion_matrix(labels, pred, counts[i])
            reduce_over_ranks(self, counts)
            matrices = list(counts.cpu().numpy())
        return self._rows(matrices)

    def score_all_groups(self, test_set, groups, max_iterations=None):
        """score_all per group of images on ONE pass of the experts: {key: what score_all returns for the images of that key}.
        groups as BaseModel.score_groups takes them: one hashable key per image in data order, or 'image'.  On the one-pass
        heads the grouped joint histogram gives both experts and Bayes; the Dirichlet and the average label maps (fused heads)
        are counted by the grouped confusion kernel.  With three or four experts the
        counting head takes the group ids itself: the three launches of score_all, a matrix per group each."""
        self._require_measurements()
        C = self.config['num_classes']
        am1, lognorm, logprior = self.dirichlet
        test_set, keys, ids = image_groups(test_set, groups, max_iterations, self.config['batchsize'],
                                           across_ranks=self.config.get('reduce_score_over_ranks', False))
        G, scored = len(keys), [0]
        if not keys:
            return {}
        if multi_head_applicable(self):
            fused = torch.zeros((3, G, 1, C, C), dtype=torch.int64, device=self.device)    # Bayes, Dirichlet, average
            experts = torch.zeros((G, len(self.modalities), C, C), dtype=torch.int64, device=self.device)
            for batch, labels, batch_ids in grouped_batches(self, test_set, ids, G, max_iterations, scored):
                self._count_multi(run_lowres_scores_multi(self, batch), labels, fused, experts, groups=batch_ids, num_groups=G)
            reduce_over_ranks(self, fused, experts)
            fused, experts = fused.cpu().numpy(), experts.cpu().numpy()
            matrices = [list(experts[g]) + [fused[i][g][0] for i in range(3)] for g in range(G)]
        elif self._two_expert_heads_applicable():
            hist = torch.zeros((G, C, C, C), dtype=torch.int64, device=self.device)
            counts = torch.zeros((2, G, C, C), dtype=torch.int64, device=self.device)      # Dirichlet, average
            for batch, labels, batch_ids in grouped_batches(self, test_set, ids, G, max_iterations, scored):
                Sa, Sb, ba, bb, n, hi, wi = run_lowres_scores(self, batch)
                ops.fused_head_joint_hist_grouped(Sa, Sb, ba, bb, n, hi, wi, C, labels, batch_ids, G, hist=hist)
                fused = ops.fused_head(Sa, Sb, ba, bb, n, hi, wi, C, am1, logprior, lognorm=lognorm)
                ops.confusion_matrix_grouped(labels, fused, batch_ids, G, cm=counts[0])
                fused = ops.fused_head_average(Sa, Sb, ba, bb, n, hi, wi, C)
                ops.confusion_matrix_grouped(labels, fused, batch_ids, G, cm=counts[1])
            reduce_over_ranks(self, hist, counts)
            hist, counts = hist.cpu().numpy(), counts.cpu().numpy()
            decision = fused_decision_table(self.bayes[0], self.bayes[1])
            matrices = [list(expert_matrices_from_joint_hist(hist[g])) + [confusion_from_joint_hist(hist[g], decision),
                                                                         counts[0][g], counts[1][g]] for g in range(G)]
        else:
            counts = torch.zeros((len(self._row_names()), G, C, C), dtype=torch.int64, device=self.device)
            for batch, labels, batch_ids in grouped_batches(self, test_set, ids, G, max_iterations, scored):
                for i, pred in enumerate(self._generic_label_maps(batch)):
                    ops.confusion_matrix_grouped(labels, pred, batch_ids, G, cm=counts[i])
            reduce_over_ranks(self, counts)
            matrices = counts.cpu().numpy().transpose(1, 0, 2, 3)
        return grouped_results(keys, ids, scored[0], matrices, complete=max_iterations is None, result=self._rows,
                               seen=groups_seen(self, ids, scored[0], G))
