"""MC-dropout variance fusion (reference: xview/models/variance_mix.py; timed by experiments/timing.py:181-218).

Per modality the FCN expert runs `num_samples` passes with dropout after pool3 and pool4 (dropout_layers=['pool3']) and one
pass without; the variance of the samples' softmax over the samples, averaged over the classes, weighs the plain pass's
probabilities: fused = sum_m prob_m / (1e-20 + var_m) / sum_m 1 / (1e-20 + var_m), label = argmax(fused).  Here the layers
before the first dropout site run once per expert, the T + 1 passes from conv4_1 on as one batch (FcnEngine.mc_lowres_scores),
and one kernel takes both experts' low-resolution scores to the fused labels (ops.variance_head)."""
from . import ops
from .basic_fusion_model import FusionModel, mc_dropout_setup, output_key, per_expert_output, run_mc_lowres_scores


def variance_fusion(probs, variances):
    """Functional entry point with the reference's signature (variance_mix.py:7-15): probs, a list of float32 CUDA tensors
    [N,H,W,C]; variances, one float32 tensor [N,H,W] (or [N,H,W,1]) per expert -> the fused score float32 [N,H,W,C]."""
    probs = [p.contiguous() for p in probs]
    shape = tuple(probs[0].shape[:-1])
    variances = [v.reshape(shape).contiguous() for v in variances]
    _, score = ops.variance_fuse(probs, variances, want_score=True, want_label=False)
    return score


class VarianceFusion(FusionModel):
    """config: num_units, num_classes (via data_description), prefixes {modality: prefix} (or modalities, a list: each its own
    prefix), num_channels, expert_model ('fcn' only, as in the reference), dropout_rate, num_samples; dropout_seed (default:
    seed, else 0); mc_chunk_images (default 64: most images one launch of the sampled layers sees).  output_attr 'fused_score',
    'probs' ([N, E, H, W, C]: the plain passes' softmax) and 'variance' ([N, E, H, W]) return the optional outputs of the head.
    Every call draws new masks (the engines' pass counters advance by num_samples), so the step is never captured into a
    hipGraph: a replay would redraw the masks of the captured call."""

    def __init__(self, output_dir=None, **config):
        standard_config = {'learning_rate': 0.0}
        standard_config.update(config)
        if 'prefixes' not in standard_config and 'modalities' in standard_config:
            standard_config['prefixes'] = {m: m for m in standard_config['modalities']}
        mc_dropout_setup('VarianceFusion', standard_config)
        standard_config['expert_model'] = 'fcn'
        FusionModel.__init__(self, 'VarianceFusion', output_dir=output_dir, **standard_config)

    agreement_refusal = ('every pass draws dropout masks and the plain passes\' labels are not what the variance head fuses: '
                         'the MC-dropout fusions are not served')

    def _build_graph(self):
        FusionModel._build_graph(self)
        if len(self.modalities) != 2:
            raise UserWarning('ERROR: VarianceFusion fuses two experts, got %d' % len(self.modalities))
        self._dropout_seed = mc_dropout_setup('VarianceFusion', self.config, engines=self.experts.values())[2]

    def _graph_capturable(self):
        return False

    def _predict_batch_impl(self, batch, output_attr=None):
        key = output_key(output_attr)
        out = ops.variance_head(*run_mc_lowres_scores(self, batch, 'mc_lowres_scores'), self.config['num_classes'],
                                int(self.config['num_samples']), want_score=key == 'fused_score', want_probs=key == 'probs',
                                want_variance=key == 'variance')
        if 'probs' in out:
            return per_expert_output(self, out['probs'], keep='probs')
        if 'variance' in out:
            return per_expert_output(self, out['variance'], keep='variances')
        if 'fused_score' in out:
            return out['fused_score']
        return out['label']
