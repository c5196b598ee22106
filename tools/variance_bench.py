#!/usr/bin/env python3
"""Inference time of the MC-dropout variance fusion model (get_model('variance_fusion')) in the protocol of the reference's
time_variance_fcn (experiments/timing.py:181-218): constant inputs [1, 384, 768, 3] and [1, 384, 768, 1] (tf.ones), the
two experts, mean +- std over repetitions, for T in {5, 10, 20} samples.

Two forms, alternated in one process on the same model (same weights, same head kernel):
  batched     the model's predict step: the layers before the first dropout site once per expert, then T + 1 passes from
              conv4_1 on as one batch (FcnEngine.mc_lowres_scores), one variance head launch;
  sequential  what the reference's graph computes: T + 1 separate passes per expert -- T with set_dropout(['pool3'], r, seed)
              + lowres_scores, one plain -- into the same low-resolution buffers, then the same variance head.
Times are host wall clock around one call ending in a device synchronise.  Prints one JSON line; --out also writes it."""
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
    return get_model('variance_fusion')(data_description=desc, num_units=U, prefixes={'rgb': 'rgb', 'depth': 'depth'},
                                        num_channels={'rgb': 3, 'depth': 1}, expert_model='fcn', dropout_rate=rate,
                                        num_samples=T, seed=1, device=str(dev))


def sequential(model, inputs, T, rate):
    """T + 1 separate passes per expert into a (T+1)-slot score buffer, then the model's head"""
    from modular_semantic_segmentation_amd import ops
    from modular_semantic_segmentation_amd.basic_fusion_model import run_trunks

    def trunk(m, st):
        eng = model.experts[m]
        key = ('seq_S', T)
        S = eng._arena.get(key)
        S0, geo = eng.lowres_scores(inputs[m])
        if S is None:
            S = eng._arena[key] = torch.zeros((T + 1,) + tuple(S0.shape[1:]), dtype=torch.float32, device=S0.device)
        S[0:1].copy_(S0)
        eng.set_dropout(['pool3'], rate, model._dropout_seed + model.modalities.index(m))
        for t in range(T):
            S[t + 1:t + 2].copy_(eng.lowres_scores(inputs[m])[0])
        eng.set_dropout([], 0.0)
        return S, geo
    res = run_trunks(model, inputs, trunk, pair=False)
    a, b = model.modalities
    n, hi, wi = res[a][1]
    return ops.variance_head(res[a][0], res[b][0], model.experts[a].b['score'], model.experts[b].b['score'], n, hi, wi, C,
                             T)['label']


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
        sys.exit('variance_bench.py needs a GPU')
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    batch = {'rgb': np.ones((1, H, W, 3), np.float32), 'depth': np.ones((1, H, W, 1), np.float32)}
    rec = {'tool': 'variance_bench', 'shape': [1, H, W], 'num_classes': C, 'num_units': U, 'rate': args.rate,
           'reps': args.reps, 'unit': 's', 'results': {}}
    for T in [int(t) for t in args.samples.split(',')]:
        model = make_model(T, args.rate, dev)
        inputs = {m: model._to_device(batch[m], torch.float32) for m in model.modalities}
        forms = {'batched': lambda: model._predict_batch(inputs),
                 'sequential': lambda: sequential(model, inputs, T, args.rate)}
        for _ in range(args.warmup):
            for f in forms.values():
                f()
        times = {k: [] for k in forms}
        for _ in range(args.reps):
            for k, f in forms.items():
                times[k].append(timed(f, dev))
        r = {k: {'mean': float(np.mean(v)), 'std': float(np.std(v)), 'min': float(np.min(v))} for k, v in times.items()}
        r['speedup'] = r['sequential']['mean'] / r['batched']['mean']
        rec['results'][str(T)] = r
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
