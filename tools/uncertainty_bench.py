#!/usr/bin/env python3
"""Inference time of the MC-dropout Bayesian FCN (get_model('bayesian_fcn')) in the protocol of tools/variance_bench.py: one
constant input [1, 384, 768, 3] (tf.ones, experiments/timing.py), mean +- std over repetitions, T in {5, 10, 20} samples at
rate 0.5, for two site lists: the reference's default (every site: replication at pool3) and ['conv4_3', 'conv5_3',
'features'] (the whole 3x3 trunk once).

Two forms, alternated in one process on the same model (same weights):
  fused       the model's step behind predict_uncertainty: what the samples share once, the samples as one batch
              (FcnEngine.mc_sample_scores), ONE head launch with every output (ops.mc_uncertainty_head);
  sequential  the only way to the same maps without it: T times set_dropout + forward(want=('prob',)), the T full-resolution
              probability tensors stacked, the label and the four maps by torch reductions on the device.
Times are host wall clock around one call ending in a device synchronise.  Prints one JSON line; --out also writes it."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
C, U, H, W = 12, 64, 384, 768
CASES = {'default': ['pool3', 'pool4', 'conv4_3', 'conv5_3', 'features'], 'trunk_once': ['conv4_3', 'conv5_3', 'features']}


def make_model(T, rate, layers, dev):
    from modular_semantic_segmentation_amd import get_model
    desc = ({'rgb': 'float32'}, {'rgb': (None, None, 3)}, C)
    return get_model('bayesian_fcn')('rgb', desc, 'rgb', dropout_layers=layers, num_units=U, dropout_rate=rate, num_samples=T,
                                     seed=1, device=str(dev))


def sequential(model, x, T, rate, layers):
    eng = model.engine
    eng.set_dropout(layers, rate, model._dropout_seed)
    samples = torch.stack([eng.forward(x, want=('prob',))['prob'] for _ in range(T)], 0)
    eng.set_dropout([], 0.0)
    mean = samples.mean(0)

    def entropy(p):
        return -(p * torch.log(p.clamp(1e-10, 1.0))).sum(-1) / math.log(C)
    return {'label': mean.argmax(-1), 'mean': mean, 'entropy': entropy(mean), 'cond_entropy': entropy(samples).mean(0),
            'variance': samples.var(0, unbiased=False).sum(-1)}


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
        sys.exit('uncertainty_bench.py needs a GPU')
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    batch = {'rgb': np.ones((1, H, W, 3), np.float32)}
    rec = {'tool': 'uncertainty_bench', 'shape': [1, H, W], 'num_classes': C, 'num_units': U, 'rate': args.rate,
           'reps': args.reps, 'unit': 's', 'cases': CASES, 'results': {}}
    for case, layers in CASES.items():
        rec['results'][case] = {}
        for T in [int(t) for t in args.samples.split(',')]:
            model = make_model(T, args.rate, layers, dev)
            x = model._to_device(batch['rgb'], torch.float32)
            forms = {'fused': lambda: model._uncertainty_of_batch({'rgb': x}, ('mean', 'entropy', 'cond_entropy', 'variance')),
                     'sequential': lambda: sequential(model, x, T, args.rate, layers)}
            for _ in range(args.warmup):
                for f in forms.values():
                    f()
            times = {k: [] for k in forms}
            for _ in range(args.reps):
                for k, f in forms.items():
                    times[k].append(timed(f, dev))
            r = {k: {'mean': float(np.mean(v)), 'std': float(np.std(v)), 'min': float(np.min(v))} for k, v in times.items()}
            r['speedup'] = r['sequential']['mean'] / r['fused']['mean']
            rec['results'][case][str(T)] = r
            del model
            torch.cuda.empty_cache()
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
