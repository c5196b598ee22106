"""IBCC fusion of the experts' label maps: a Bayes fusion whose confusion matrices keep learning on the UNLABELLED data it
fuses (reference: experiments/ibcc_fusion.py, which only dumps the label maps for an external IBCC; ibcc.py is that IBCC)."""
import numpy as np
import torch

from . import ops
from .base_model import (BaseModel, grouped_batches, groups_seen, image_groups, iterate_batches, reduce_over_ranks,
                         score_measures)
from .basic_fusion_model import (FusionModel, _labelled_batches, output_key, run_experts, run_lowres_scores,
                                 run_lowres_scores_multi, tuple_head_applicable)
from .bayes_mix import BayesFusion
from .ibcc import ibcc_priors, vb_ibcc


class IbccFusion(BayesFusion):
    """config: as BayesFusion (confusion_matrices {modality: [C,C] label x pred} measured on a labelled set, prefixes,
    num_channels, num_units, expert_model, ...) plus prior_strength (None: the measured pixels count as observations; a number
    s: every true-class row counts as s pseudo-observations -- ibcc.ibcc_priors), ibcc_max_iter (200) and ibcc_tol (1e-6) of
    the variational updates.

    The fused label of a pixel is lut[t], t the tuple of the experts' labels.  Before adapt() the table is the priors' own
    decision; adapt(data) counts the tuple histogram of `data` -- no labels are read -- and replaces it by the decision of
    the variational posterior.  Where two to four commuted FCN experts run with the fused head and ops.tuple_capacity serves
    the pair (tuple_head_applicable), predict / score / score_groups / adapt stop the trunks at their low-resolution scores and
    run ONE label-tuple head per batch; otherwise the experts' label maps are materialised and looked up in torch.  Both routes
    give the same integers."""

    def __init__(self, output_dir=None, confusion_matrices=False, **config):
        standard_config = {'prior_strength': None, 'ibcc_max_iter': 200, 'ibcc_tol': 1e-6}
        standard_config.update(config)
        if standard_config.get('decision_matrix', False):
            raise ValueError('IbccFusion always decides through its own lookup table: decision_matrix is BayesFusion\'s')
        # the priors count the measured pixels: kept in float64, label x pred (BayesFusion holds float32 transposes, exact
        # only up to 2^24 per cell)
        self.measured = {m: np.asarray(cm, np.float64) for m, cm in (confusion_matrices or {}).items()}
        BayesFusion.__init__(self, output_dir=output_dir, confusion_matrices=confusion_matrices, **standard_config)
        self.name = 'IbccFusion'

    def _build_graph(self):
        BayesFusion._build_graph(self)
        self.alpha0, self.nu0 = ibcc_priors([self.measured[m] for m in self.modalities], self.config['prior_strength'])
        self.ibcc_prior = self._solve(np.zeros(self.config['num_classes'] ** len(self.modalities)))
        self.use_adaptation(self.ibcc_prior)

    def _solve(self, hist):
        return vb_ibcc(hist, self.alpha0, self.nu0, max_iter=self.config['ibcc_max_iter'], tol=self.config['ibcc_tol'])

    def use_adaptation(self, result):
        """Decide by `result` (an ibcc.IbccResult: what adapt() returned, one key's entry of a grouped adapt(), or
        self.ibcc_prior) from now on."""
        T, C = self.config['num_classes'] ** len(self.modalities), self.config['num_classes']
        if result.lut.shape != (T,) or result.posterior.shape != (T, C):
            raise ValueError('an IBCC result over %d tuples, this model has %d' % (len(result.lut), T))
        self.ibcc = result
        self.lut = torch.from_numpy(np.ascontiguousarray(result.lut, np.uint8)).to(self.device)
        with np.errstate(divide='ignore'):
            self.log_posterior = torch.from_numpy(np.log(result.posterior).astype(np.float32)).to(self.device)
        self._graph = None          # a captured step replays the old table

    # ---- the fused heads of BayesFusion decide by its float32 log-likelihood sums: not this model's decision -----------------
    def _fused_head(self):
        return None

    def _multi_head(self):
        return None

    def _agreement_head(self):
        return None                 # score_agreement fuses the materialised maps through _fusion and ops.agreement_table

    calibration_refusal = ('an IBCC fusion decides by a lookup over the experts\' label tuple; its posterior per tuple is not '
                           'a per-pixel class score the calibration kernels take')

    def _lowres(self, batch):
        """(scores, biases, n, hi, wi) of the label-tuple heads; two experts share their paired launches as in every route."""
        if len(self.modalities) == 2:
            Sa, Sb, ba, bb, n, hi, wi = run_lowres_scores(self, batch)
            return [Sa, Sb], [ba, bb], n, hi, wi
        return run_lowres_scores_multi(self, batch)

    def _tuples(self, expert_outputs):
        """int64 tuple index of every pixel from the experts' materialised label maps."""
        C = self.config['num_classes']
        t = None
        for m in self.modalities:
            label = expert_outputs[m]['classification']
            t = label if t is None else t * C + label
        return t

    def _fusion(self, expert_outputs, output_attr=None):
        t = self._tuples(expert_outputs)
        self.probs = {m: expert_outputs[m].get('prob') for m in self.modalities}
        if output_attr == 'fused_score':
            return self.log_posterior[t]
        if output_attr == 'probs':
            return torch.stack([self.probs[m] for m in self.modalities], 1)
        return self.lut[t].to(torch.int64)

    def _predict_batch_impl(self, batch, output_attr=None):
        if output_attr is None and tuple_head_applicable(self):
            self.expert_outputs = None
            return ops.fused_head_multi_lut(*self._lowres(batch), self.config['num_classes'], self.lut)
        key = output_key(output_attr)
        wants = self.expert_wants + (('prob',) if key == 'probs' else ())
        self.expert_outputs = run_experts(self, batch, wants)
        return self._fusion(self.expert_outputs, output_attr=key)

    # ---- scoring: the counting form of the lookup head ---------------------------------------------------------------------
    def score(self, data, max_iterations=None):
        if not tuple_head_applicable(self):
            return BaseModel.score(self, data, max_iterations)
        C = self.config['num_classes']
        cm = torch.zeros((C, C), dtype=torch.int64, device=self.device)
        for batch, labels in _labelled_batches(self, data, max_iterations):
            ops.fused_head_multi_lut_count(*self._lowres(batch), C, self.lut, labels, cm=cm)
        reduce_over_ranks(self, cm)
        cm = cm.cpu().numpy().astype(np.float64)
        return score_measures(cm), cm

    def _count_groups(self, data, ids, num_groups, max_iterations, scored):
        if not tuple_head_applicable(self):
            return FusionModel._count_groups(self, data, ids, num_groups, max_iterations, scored)
        C = self.config['num_classes']
        cm = torch.zeros((num_groups, C, C), dtype=torch.int64, device=self.device)
        for batch, labels, batch_ids in grouped_batches(self, data, ids, num_groups, max_iterations, scored):
            ops.fused_head_multi_lut_count(*self._lowres(batch), C, self.lut, labels, groups=batch_ids, num_groups=num_groups,
                                           cm=cm)
        reduce_over_ranks(self, cm)
        return cm.cpu().numpy()

    def score_grid(self, data, search_parameters, max_iterations=None):
        raise NotImplementedError('IbccFusion.score_grid: the class prior and the confusion matrices of an IBCC fusion are '
                                  'posterior quantities that adapt() learns, not parameters to search; build one model per '
                                  'prior_strength with experiments.grid_search')

    # ---- measurement and adaptation -----------------------------------------------------------------------------------------
    def measure(self, measure_set):
        """Every expert's confusion matrix {modality: float64 [C,C] label x pred} from ONE pass of the experts over the
        LABELLED `measure_set` (experiments/bayes_fusion.py:146-195 scores one model per expert).  The priors are rebuilt from
        them and the model decides by those priors: an earlier adaptation is dropped."""
        C = self.config['num_classes']
        cms = {m: torch.zeros((C, C), dtype=torch.int64, device=self.device) for m in self.modalities}
        for batch, labels in _labelled_batches(self, measure_set, None):
            outs = run_experts(self, batch, ('classification',))
            for m in self.modalities:
                ops.confusion_matrix(labels, outs[m]['classification'].contiguous(), cms[m])
        reduce_over_ranks(self, *cms.values())
        matrices = {m: cms[m].cpu().numpy().astype(np.float64) for m in self.modalities}
        self.measured = dict(matrices)
        self.confusion_matrices = {m: matrices[m].astype('float32').T for m in self.modalities}    # as BayesFusion holds them
        self._initialize_graph()
        return matrices

    def _count_tuples(self, data, ids, num_groups, max_iterations, scored):
        """int64 [G, T] on the host: every group's tuple histogram from ONE pass of the experts over `data`, whose labels --
        if it has any -- are not read.  ids None: one group, every image."""
        C, T = self.config['num_classes'], self.config['num_classes'] ** len(self.modalities)
        hist = torch.zeros((num_groups, T), dtype=torch.int64, device=self.device)
        dev_ids = None if ids is None else ops.upload_group_ids(ids, num_groups, self.device)
        fused_route = tuple_head_applicable(self)
        for batch in self._device_batches(iterate_batches(data, self.config['batchsize'], max_iterations), labels=False):
            n = len(batch[self.modalities[0]])
            if ids is not None and scored[0] + n > len(ids):
                raise ValueError('groups names %d images, the data holds more' % len(ids))
            batch_ids = None if ids is None else dev_ids[scored[0]:scored[0] + n]
            if fused_route:
                into = dict(hist=hist[0]) if batch_ids is None else dict(groups=batch_ids, num_groups=num_groups, hist=hist)
                ops.fused_head_multi_tuple_hist(*self._lowres(batch), C, **into)
            else:
                t = self._tuples(run_experts(self, batch, ('classification',))).reshape(n, -1)
                if batch_ids is not None:
                    t = t + batch_ids.to(torch.int64)[:, None] * T
                hist += torch.bincount(t.reshape(-1), minlength=num_groups * T).reshape(num_groups, T)
            scored[0] += n
        reduce_over_ranks(self, hist)
        return hist.cpu().numpy()

    def adapt(self, data, max_iterations=None, groups=None):
        """Adapt to `data` without labels: one pass of the experts counts the histogram of their label tuples (summed over
        the ranks under reduce_score_over_ranks), ibcc.vb_ibcc updates every expert's confusion matrix and the class
        proportions from the priors on it, and the model decides by the result (self.ibcc) from now on; returns it.  Calling
        it again adapts from the priors on the new data.  max_iterations bounds the batches read, as in score().

        groups -- one hashable key per image in data order, or 'image', as score_groups takes them -- returns {key: result},
        each the result of adapt() on the images of that key alone, from the same pass (one adapted model per sequence:
        use_adaptation(result) installs one); the model itself then decides by the adaptation to ALL the images."""
        if groups is None:
            result = self._solve(self._count_tuples(data, None, 1, max_iterations, [0])[0])
            self.use_adaptation(result)
            return result
        data, keys, ids = image_groups(data, groups, max_iterations, self.config['batchsize'],
                                       across_ranks=self.config.get('reduce_score_over_ranks', False))
        if not keys:
            return {}
        scored = [0]
        hists = self._count_tuples(data, ids, len(keys), max_iterations, scored)
        if max_iterations is None and scored[0] != len(ids):
            raise ValueError('groups names %d images, the data holds %d' % (len(ids), scored[0]))
        seen = groups_seen(self, ids, scored[0], len(keys))
        self.use_adaptation(self._solve(hists.sum(0)))
        return {keys[g]: self._solve(hists[g]) for g in np.flatnonzero(seen).tolist()}
