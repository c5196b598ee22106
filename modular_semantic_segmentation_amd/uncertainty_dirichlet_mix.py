"""Uncertainty-weighted Dirichlet fusion (reference: xview/models/uncertainty_dirichlet_mix.py).

Two FCN experts are fused with class-conditional Dirichlets as in dirichlet_mix, but every expert's parameters are softened
per pixel by that expert's MC-dropout variance.  Per expert e, with C classes, T = num_samples and r = dropout_rate:

  samples    x_t = x with whole PIXELS dropped (one Bernoulli(1 - r) draw per image, row and column, shared by the input
             channels; kept pixels times 1 / (1 - r)), p_t = softmax(fcn(x_t)), t = 1 .. T; the plain pass p = softmax(fcn(x))
  variance   v[c] = population variance of p_t[c] over t, per pixel and class
  mix        mean_c v[c] / max v -- the maximum over EVERY pixel, class and image of the expert's tensor in that call (a quirk
             of the reference kept on purpose: a prediction depends on what else is in its batch)
  alpha      alpha[j, c] = A_e[j, c] (1 - mix) + mix (1 + delta_jc), A_e the fitted [C, C] parameters (params[k, c] as in
             dirichlet_mix), the standard parameters ones plus the identity
  ll_e[c]    sum_j (alpha[j, c] - 1) log(1e-20 + p[j] / sum p) + lgamma(sum_j alpha[j, c]) - sum_j lgamma(alpha[j, c])

and score[c] = ll_0[c] + ll_1[c] + log(1e-20 + prior[c]), label = argmax (lowest index on ties).

Deviation from the reference, which divides 0 / 0 where max v = 0: num_samples < 2 and dropout_rate == 0 (no variance at
all) raise ValueError when the model is built, and a maximum that is still exactly 0 at run time gives mix = 0, the plain
Dirichlet fusion.

All T + 1 trunks of an expert run (the dropout site is the input: FcnEngine.mc_input_scores); one kernel takes both experts'
low-resolution scores to mvar = mean_c v and max v (ops.uncertainty_moments), a second one to the fused labels
(ops.uncertainty_dirichlet_head)."""
import numpy as np
import torch

from . import ops
from .basic_fusion_model import FusionModel, device_tables, mc_dropout_setup, per_expert_output, run_mc_lowres_scores
from .dirichlet_mix import DirichletFusion, class_prior_vector


def _tables(conditional_params, prior, device):
    params = np.ascontiguousarray(np.stack([np.asarray(A, np.float32) for A in conditional_params]), np.float32)
    if params.ndim != 3 or params.shape[0] != 2 or params.shape[1] != params.shape[2]:
        raise ValueError('two [C, C] parameter matrices, got an array of shape %s' % (params.shape,))
    C = params.shape[1]
    prior = np.broadcast_to(np.asarray(prior, np.float32), (C,))
    logprior = np.log(np.float32(1e-20) + prior, dtype=np.float32)
    return device_tables(device, params, np.ascontiguousarray(logprior))


def dirichlet_uncertainty_fusion(probs, conditional_params, uncertainties, prior):
    """Functional entry point with the reference's signature (uncertainty_dirichlet_mix.py:18-52): probs, two float32 CUDA
    tensors [N,H,W,C] (renormalised inside the kernel); conditional_params, two [C,C] arrays (params[k, c]); uncertainties, two
    non-negative float32 tensors [N,H,W,C] (per-class variances); prior, [C] probabilities (or one value) -> the fused score
    float32 [N,H,W,C].  ops.uncertainty_weights per expert, then ops.uncertainty_dirichlet_fuse."""
    probs = [p.contiguous() for p in probs]
    if len(probs) != 2 or len(uncertainties) != 2:
        raise ValueError('dirichlet_uncertainty_fusion fuses two experts')
    shape = tuple(probs[0].shape[:-1])
    dev = probs[0].device
    mvar = torch.empty((2,) + shape, dtype=torch.float32, device=dev)
    vmax = torch.empty(2, dtype=torch.float32, device=dev)
    for e, u in enumerate(uncertainties):
        ops.uncertainty_weights(u.contiguous(), mvar=mvar[e], vmax=vmax[e:e + 1])
    params, logprior = _tables(conditional_params, prior, dev)
    _, score = ops.uncertainty_dirichlet_fuse(probs, mvar, vmax, params, logprior, want_score=True, want_label=False)
    return score


class UncertaintyMix(DirichletFusion):
    """config: modalities (two; the expert of modality m uses prefix m), num_channels, num_units, expert_model ('fcn' only),
    class_prior, delta, beta, dropout_rate (in (0, 1)), num_samples (at least 2); optional dirichlet_params {modality: [C,C],
    'class_counts': [C]}, dropout_seed (default: seed, else 0), mc_chunk_images (default 64: most images one launch of the
    sampled trunks sees).  There is no sigma.  fit() is DirichletFusion's (plain passes, the same statistics and Newton fit).

    predict returns the label; output_attr 'fused_score' ([N,H,W,C]), 'probs' ([N,E,H,W,C]: the plain passes' softmax),
    'variance' ([N,E,H,W]: mean_c v) and 'mix' ([N,E,H,W]) return the optional outputs.  mix divides by the maximum variance
    of the BATCH (see the module text), so predictions depend on how predict batches; a maximum of exactly 0 gives mix = 0
    where the reference divides 0 / 0.  Every call draws new masks (the engines' pass counters advance by num_samples), so the
    step is never captured into a hipGraph: a replay would redraw the masks of the captured call."""

    def __init__(self, output_dir=None, **config):
        mc_dropout_setup('UncertaintyMix', config, strict=True)
        if len(config['modalities']) != 2:
            raise UserWarning('ERROR: UncertaintyMix fuses two experts, got %d' % len(config['modalities']))
        if config.get('conv_dtype', 'bf16') != 'bf16':
            raise NotImplementedError('UncertaintyMix needs the bf16 engine: the fp8 / fp32 engines are not sampled')
        config = dict(config, expert_model='fcn')
        DirichletFusion.__init__(self, output_dir=output_dir, **config)
        self.name = 'UncertaintyMix'

    agreement_refusal = ('every pass draws dropout masks and the plain passes\' labels are not what the uncertainty head fuses: '
                         'the MC-dropout fusions are not served')

    def _build_graph(self):
        FusionModel._build_graph(self)
        self._dropout_seed = mc_dropout_setup('UncertaintyMix', self.config, strict=True, engines=self.experts.values())[2]
        if hasattr(self, 'dirichlet_params'):
            C = self.config['num_classes']
            prior = class_prior_vector(self.class_counts, self.config['class_prior'], C)
            self.params_dev, self.logprior = _tables([self.dirichlet_params[m] for m in self.modalities], prior, self.device)
        else:
            self.prediction = 0      # no fusion possible before fit()

    def _graph_capturable(self):
        return False

    def _predict_batch_impl(self, batch, output_attr=None):
        if not hasattr(self, 'params_dev'):
            raise UserWarning('ERROR: UncertaintyMix has no measurements yet, call fit() first')
        key = 'label' if output_attr is None else output_attr
        if key not in ('label', 'fused_score', 'probs', 'variance', 'mix'):
            raise UserWarning('ERROR: UncertaintyMix has no output %r' % output_attr)
        scores = run_mc_lowres_scores(self, batch, 'mc_input_scores')
        C = self.config['num_classes']
        mvar, vmax = ops.uncertainty_moments(*scores, C, int(self.config['num_samples']))
        if key == 'variance':
            return per_expert_output(self, mvar, keep='variances')
        out = ops.uncertainty_dirichlet_head(*scores, C, mvar, vmax, self.params_dev, self.logprior,
                                             want_score=key == 'fused_score', want_probs=key == 'probs', want_mix=key == 'mix')
        if key in ('probs', 'mix'):
            return per_expert_output(self, out[key], keep='probs' if key == 'probs' else None)
        return out[key]
