"""MC-dropout Bayesian FCN (reference: xview/models/bayesian_fcn.py, after Kendall et al., arXiv 1511.02680).

ONE FCN expert runs `num_samples` passes with dropout at the listed sites (simple_fcn.py:51-63,69-78,124-126); the prediction is
the argmax of the MEAN of the T softmaxes, and three per-pixel uncertainty maps come with it (bayesian_fcn.py:48-57,
custom_layers.py:251-256):

    mean         = (1/T) sum_t p_t                                                [N,H,W,C]
    entropy      = -sum_c mean_c ln(clip(mean_c, 1e-10, 1)) / ln C                [N,H,W]   (normed to [0,1])
    cond_entropy = (1/T) sum_t ( -sum_c p_tc ln(clip(p_tc, 1e-10, 1)) / ln C )    [N,H,W]
    variance     = sum_c ( (1/T) sum_t p_tc^2 - ((1/T) sum_t p_tc)^2 )            [N,H,W]

Here what the samples share runs once, the samples run as one batch from the earliest active dropout site on
(FcnEngine.mc_sample_scores), and one kernel takes the T low-resolution score maps to the label and the maps
(ops.mc_uncertainty_head): nothing of size T x C per pixel is written to HBM."""
import numpy as np
import torch

from . import ops
from .base_model import iterate_batches
from .basic_fusion_model import mc_dropout_setup
from .simple_fcn import SimpleFCN
from .uncertainty_model import UncertaintyModel

OUTPUTS = ('label', 'mean', 'entropy', 'cond_entropy', 'variance')


def sampling_uncertainty(inputs, pipeline, num_samples, num_classes, **kwargs):
    """Functional entry point with the reference's signature (bayesian_fcn.py:9-57): calls pipeline(inputs, **kwargs)['prob']
    (float32 CUDA tensor [N,H,W,C]; e.g. simple_fcn.fcn with dropout arguments -- every call draws new masks) num_samples
    times and reduces the stacked samples with xv_sampling_uncertainty -> (mean [N,H,W,C], {'entropy', 'cond_entropy',
    'variance'}, each [N,H,W])."""
    T = int(num_samples)
    if T < 1:
        raise ValueError('num_samples must be at least 1')
    samples = None
    for t in range(T):
        prob = pipeline(inputs, **kwargs)['prob']
        if prob.shape[-1] != num_classes:
            raise ValueError('the pipeline returns %d classes, num_classes is %d' % (prob.shape[-1], num_classes))
        if samples is None:
            samples = torch.empty((T,) + tuple(prob.shape), dtype=torch.float32, device=prob.device)
        samples[t].copy_(prob)          # (a pipeline may hand out the same buffer every call)
    out = ops.sampling_uncertainty(samples, want_label=False)
    return out['mean'], {k: out[k] for k in ('entropy', 'cond_entropy', 'variance')}


class BayesianFCN(UncertaintyModel, SimpleFCN):
    """Args as the reference: prefix, data_description, modality, output_dir, dropout_layers (default: every site), **config
    with required `num_units`, `dropout_rate`, `num_samples`; optional `method` ('sampling', the only one), `dropout_seed`
    (default: `seed`, else 0), `mc_chunk_images` (default 64: most images one launch of the sampled layers sees).  Variables,
    import and export are SimpleFCN's: weights exported by get_model('fcn') load unchanged.

    predict(data) returns the label of the mean; output_attr 'mean' (alias 'prob': [N,H,W,C]), 'entropy', 'cond_entropy',
    'variance' ([N,H,W]) return one map; predict_uncertainty(data) returns all of them from ONE set of masks.  Every call
    draws new masks (the engine's pass counter advances by num_samples), so the step is never captured into a hipGraph: a
    replay would redraw the masks of the captured call.

    The uncertainty benchmarks are UncertaintyModel's (uncertainty_model.py: misclassification_detection_score,
    out_of_distribution_detection_score, nll_score, value_distribution, uncertainty_tables, temperature_search); a batch goes
    through the scoring form of the head (ops.mc_uncertainty_score), which bins the three metrics and sums the NLL where the
    head above stores its maps.  Optional `temperature_scaling` (default 1; custom_layers.py:239-248) divides the logits of
    the benchmarks; predict() / predict_uncertainty() raise NotImplementedError under another value: the map-writing head has
    no temperature, and the key is never ignored silently.

    Inference only: fit() raises NotImplementedError.  The reference trains this model WITH dropout (is_training=True: masks
    in the forward pass and their gradient in the backward pass), which the trainer does not do yet; train the same weights as
    get_model('fcn') and import them, or wait for that work -- this class never trains silently without dropout."""

    def __init__(self, prefix, data_description, modality, output_dir=None,
                 dropout_layers=['pool3', 'pool4', 'conv4_3', 'conv5_3', 'features'], **config):
        mc_dropout_setup('BayesianFCN', config, fusion=False)
        standard_config = {'method': 'sampling', 'batch_normalization': False, 'learning_rate': 0.0}
        standard_config.update(config)
        if standard_config['method'] != 'sampling':
            raise UserWarning("ERROR: BayesianFCN method %r not implemented ('sampling' only)" % standard_config['method'])
        SimpleFCN.__init__(self, prefix, data_description, modality, output_dir=output_dir,
                           dropout_layers=list(dropout_layers), **standard_config)

    def _build_graph(self):
        if self.config['batch_normalization'] or self.config.get('conv_dtype', 'bf16') != 'bf16':
            raise NotImplementedError('BayesianFCN needs the bf16 engine with the commuted decoder head (bilinear x8 deconv, '
                                      'no batch norm shift before its relu): batch_normalization=True and the fp8 / fp32 '
                                      'engines are not sampled')
        SimpleFCN._build_graph(self)
        self._dropout_seed = mc_dropout_setup('BayesianFCN', self.config, fusion=False, engines=[self.engine])[2]

    def _graph_capturable(self):
        return False

    calibration_refusal = ('every pass draws dropout masks and the model decides by the mean of its samples, not by one '
                           'pass\'s class scores: its confidence is scored by the uncertainty benchmarks (nll_score, temperature_search)')

    def fit(self, *args, **kwargs):
        raise NotImplementedError('BayesianFCN is inference only: training with dropout (masks in the forward pass and their '
                                  "gradient in the trainer) is not implemented; train get_model('fcn') and import its weights")

    def _train_batch(self, batch):
        self.fit()

    def _sample_scores(self, batch):
        x = self._to_device(batch[self.modality], torch.float32)
        return self.engine.mc_sample_scores(x, int(self.config['num_samples']), float(self.config['dropout_rate']),
                                            self._dropout_seed, self.config['dropout_layers'])

    # ---- UncertaintyModel: the fused scoring head -------------------------------------------------------------------------------
    def _uncertainty_maps(self, batch):
        return self._uncertainty_of_batch(batch, OUTPUTS)

    def _uncertainty_state(self, batch):
        return self._sample_scores(batch)

    def _uncertainty_accumulate(self, state, labels, tables, temperature, fixed_row):
        S, (n, hi, wi) = state
        m, o = self._uncertainty_bins()
        ops.mc_uncertainty_score(S, self.engine.b['score'], n, hi, wi, self.config['num_classes'], int(self.config['num_samples']),
                                 labels=labels, temperature=temperature, fixed_row=fixed_row, mantissa_bits=m, octaves=o,
                                 tables=tables)

    def _uncertainty_of_batch(self, batch, want):
        if float(self.config.get('temperature_scaling', 1)) != 1.0:
            raise NotImplementedError('BayesianFCN: temperature_scaling=%r applies to the uncertainty benchmarks only '
                                      '(uncertainty_tables, temperature_search, ...); the head that writes label and maps has '
                                      'no temperature, so predict() / predict_uncertainty() need temperature_scaling=1'
                                      % (self.config['temperature_scaling'],))
        S, (n, hi, wi) = self._sample_scores(batch)
        return ops.mc_uncertainty_head(S, self.engine.b['score'], n, hi, wi, self.config['num_classes'],
                                       int(self.config['num_samples']), want_mean='mean' in want,
                                       want_entropy='entropy' in want, want_cond_entropy='cond_entropy' in want,
                                       want_variance='variance' in want)

    def _predict_batch_impl(self, batch, output_attr=None):
        key = {'prob': 'mean', 'probs': 'mean', None: 'label', 'classification': 'label', 'prediction': 'label'}.get(
            output_attr, output_attr)
        if key not in OUTPUTS:
            raise UserWarning('ERROR: BayesianFCN has no output %r (one of %s)' % (output_attr, ', '.join(OUTPUTS)))
        out = self._uncertainty_of_batch(batch, (key,))
        if key != 'label':
            setattr(self, key, out[key])
        return out[key]

    def predict_uncertainty(self, data):
        """{'label' int64 [N,H,W], 'mean' float32 [N,H,W,C], 'entropy', 'cond_entropy', 'variance' float32 [N,H,W]} of `data`,
        all from the same dropout masks: one head launch per batch with every output pointer set."""
        parts = {k: [] for k in OUTPUTS}
        for batch in iterate_batches(data, self.config['batchsize']):
            out = self._uncertainty_of_batch(batch, OUTPUTS)
            for k in OUTPUTS:
                parts[k].append(out[k].cpu().numpy())
        return {k: np.concatenate(v) for k, v in parts.items()}
