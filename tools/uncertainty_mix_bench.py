#!/usr/bin/env python3
"""Inference time of the uncertainty-weighted Dirichlet fusion model (get_model('uncertainty_mix')) in the protocol of the
reference's timing experiments (experiments/timing.py; tools/variance_bench.py): constant inputs [1, 384, 768, 3] and [1, 384,
768, 1] (tf.ones), the two experts, mean +- std over repetitions, for T in {5, 10, 20} samples.

Two forms, alternated in one process on the same model (same weights):
  fused     the model's predict step: FcnEngine.mc_input_scores per expert (pixel dropout kernel, T + 1 trunks in batches), the
            moments kernel, the fusion head kernel;
  composed  the same result from what the library had before: per expert T + 1 forward(want=('prob',)) passes on inputs dropped
            by torch (one Bernoulli draw per pixel), the moments by torch reductions, and the mix / parameter / likelihood /
            score steps with torch.lgamma on the device.
The trunk passes are the same work in both forms, so the part after them is timed on its own as well (`head`): moments kernel
+ fusion head on ready low-resolution scores against the torch reductions + torch.lgamma on ready probabilities (the composed
side does not pay for its T + 1 decoder heads there).  Times are host wall clock around one call ending in a device
synchronise.  Prints one JSON line; --out also writes it."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
C, U, H, W = 12, 64, 384, 768


def make_model(T, rate, dev):
    from modular_semantic_segmentation_amd import get_model
    desc = ({'rgb': 'float32', 'depth': 'float32'}, {'rgb': (None, None, 3), 'depth': (None, None, 1)}, C)
    rng = np.random.default_rng(5)
    params = {m: (0.3 + 2 * rng.random((C, C)) + 8 * np.eye(C)).astype(np.float32) for m in ('rgb', 'depth')}
    params['class_counts'] = rng.integers(1, 1000, C)
    net = get_model('uncertainty_mix')(data_description=desc, modalities=['rgb', 'depth'], num_units=U,
                                       num_channels={'rgb': 3, 'depth': 1}, expert_model='fcn', class_prior='data', delta=1e-2,
                                       beta=1e-2, dropout_rate=rate, num_samples=T, seed=1, dirichlet_params=params,
                                       device=str(dev))
    # constant inputs through random initialisers: keep the activations alive (the recipe of the MC models' tests)
    w = dict(net.variables)
    for k in w:
        if k.endswith('/kernel') and 'upscore' not in k and 'conv1_1' not in k:
            w[k] = w[k] * 1.6
    net.variables.update(w)
    net._variables_changed()
    return net


def torch_fusion(probs, samples, params, logprior):
    """moments by torch reductions, then the mix / parameter / likelihood / score steps with torch.lgamma (float32, device)"""
    std = torch.ones((C, C), device=params.device) + torch.eye(C, device=params.device)
    score = logprior
    for e in range(2):
        v = samples[e].var(0, unbiased=False)
        mix = (v.mean(-1) / v.amax())[..., None, None]
        alpha = params[e] * (1 - mix) + mix * std
        p = probs[e] / probs[e].sum(-1, keepdim=True)
        ll = ((alpha - 1) * torch.log(1e-20 + p)[..., :, None]).sum(-2) + torch.lgamma(alpha.sum(-2)) - torch.lgamma(alpha).sum(-2)
        score = score + ll
    return score.argmax(-1)


def composed_passes(model, inputs, T, rate):
    probs, samples = [], []
    for m in model.modalities:
        eng, x = model.experts[m], inputs[m]
        smp = []
        for _ in range(T):
            keep = (torch.rand(x.shape[:3] + (1,), device=x.device) >= rate).float() * (1.0 / (1.0 - rate))
            smp.append(eng.forward(x * keep, want=('prob',))['prob'].clone())
        samples.append(torch.stack(smp, 0))
        probs.append(eng.forward(x, want=('prob',))['prob'].clone())
    return probs, samples


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--samples', default='5,10,20', help='comma-separated sample counts T')
    ap.add_argument('--rate', type=float, default=0.5)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None, help='also write the JSON record here')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('uncertainty_mix_bench.py needs a GPU')
    from modular_semantic_segmentation_amd import ops
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    batch = {'rgb': np.ones((1, H, W, 3), np.float32), 'depth': np.ones((1, H, W, 1), np.float32)}
    rec = {'tool': 'uncertainty_mix_bench', 'shape': [1, H, W], 'num_classes': C, 'num_units': U, 'rate': args.rate,
           'reps': args.reps, 'unit': 's', 'results': {}}
    for T in [int(t) for t in args.samples.split(',')]:
        model = make_model(T, args.rate, dev)
        inputs = {m: model._to_device(batch[m], torch.float32) for m in model.modalities}
        a, b = model.modalities
        bias = (model.experts[a].b['score'], model.experts[b].b['score'])
        # ready inputs of the head-only forms
        S = [model.experts[m].mc_input_scores(inputs[m], T, args.rate, i)[0].clone() for i, m in enumerate(model.modalities)]
        probs, samples = composed_passes(model, inputs, T, args.rate)

        def fused_head():
            mvar, vmax = ops.uncertainty_moments(S[0], S[1], bias[0], bias[1], 1, H // 8, W // 8, C, T)
            return ops.uncertainty_dirichlet_head(S[0], S[1], bias[0], bias[1], 1, H // 8, W // 8, C, mvar, vmax,
                                                  model.params_dev, model.logprior)['label']

        forms = {'fused': lambda: model._predict_batch(inputs),
                 'composed': lambda: torch_fusion(*composed_passes(model, inputs, T, args.rate), model.params_dev, model.logprior),
                 'fused_head': fused_head,
                 'composed_head': lambda: torch_fusion(probs, samples, model.params_dev, model.logprior)}
        for _ in range(args.warmup):
            for f in forms.values():
                f()
        times = {k: [] for k in forms}
        for _ in range(args.reps):
            for k, f in forms.items():
                times[k].append(timed(f, dev))
        r = {k: {'mean': float(np.mean(v)), 'std': float(np.std(v)), 'min': float(np.min(v))} for k, v in times.items()}
        r['speedup'] = r['composed']['mean'] / r['fused']['mean']
        r['head_speedup'] = r['composed_head']['mean'] / r['fused_head']['mean']
        rec['results'][str(T)] = r
        del model, S, probs, samples
        torch.cuda.empty_cache()
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
