#!/usr/bin/env python3
"""Cost of the fused average head and of the one-pass fusion comparison at 768x384 RGB-D, C = 12, in one process:
  (a) AverageFusion.predict on 16 resident images, the fused default path against fused_head=False (the path of the commit
      before the head existed, unchanged), alternated; and the head launch alone beside the three launches it replaces (two
      decoder heads writing `prob` + xv_average_fuse) on the same low-resolution scores;
  (b) experiments.fit_and_evaluate_all_fusions on 16 + 16 synthetic images against the sum of the per-model flows:
      fit_and_evaluate_bayes_fusion, fit_and_evaluate_dirichlet_fusion and an AverageFusion's score().
Device times by events around each form for (a) (mean / min / std over repetitions), wall-clock seconds for the flows of (b):
they build models, import weights and fit on the host, and that is part of what a user waits for.
Prints one JSON line; --out also writes it (profiles/fusion_compare_bench.json)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
C, U, H, W, N = 12, 64, 384, 768, 16


def event_time(fn, dev):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) * 1e-3


def wall_time(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0


def stats(v):
    return {'mean': float(np.mean(v)), 'min': float(np.min(v)), 'std': float(np.std(v))}


def alternate(forms, dev, warmup, reps, timer=event_time):
    for _ in range(warmup):
        for f in forms.values():
            f()
    times = {k: [] for k in forms}
    for _ in range(reps):
        for k, f in forms.items():
            times[k].append(timer(f, dev))
    return {k: stats(v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--flow-reps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None, help='also write the JSON record here')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('fusion_compare_bench.py needs a GPU')
    from modular_semantic_segmentation_amd import experiments, get_model, ops
    from modular_semantic_segmentation_amd.basic_fusion_model import run_lowres_scores
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    rng = np.random.default_rng(0)

    def images(n):
        return {'rgb': torch.from_numpy(rng.integers(0, 256, (n, H, W, 3)).astype(np.float32)).to(dev),
                'depth': torch.from_numpy(rng.integers(0, 65536, (n, H, W, 1)).astype(np.float32)).to(dev),
                'labels': torch.from_numpy(rng.integers(-1, C, (n, H, W)).astype(np.int32)).to(dev)}
    measure, test = images(N), images(N)
    desc = ({'labels': 'int32', 'rgb': 'float32', 'depth': 'float32'},
            {'labels': (None, None), 'rgb': (None, None, 3), 'depth': (None, None, 1)}, C)
    common = dict(num_units=U, num_channels={'rgb': 3, 'depth': 1}, expert_model='fcn', batchsize=N, class_prior='data', seed=1,
                  device=str(dev))
    prefixes = {'rgb': 'rgb', 'depth': 'depth'}
    rec = {'tool': 'fusion_compare_bench', 'shape': [N, H, W], 'num_classes': C, 'reps': args.reps, 'flow_reps': args.flow_reps,
           'unit': 's'}

    # ---- (a) AverageFusion.predict, fused against unfused, and the head alone
    fused = get_model('average_fusion')(data_description=desc, prefixes=prefixes, **common)
    unfused = get_model('average_fusion')(data_description=desc, prefixes=prefixes, fused_head=False, **common)
    unfused.variables.update(fused.variables)
    unfused._variables_changed()
    inputs = {k: v for k, v in test.items() if k != 'labels'}
    assert np.array_equal(fused.predict(inputs), unfused.predict(inputs))
    r = alternate({'fused': lambda: fused._predict_batch_impl(inputs), 'unfused': lambda: unfused._predict_batch_impl(inputs)},
                  dev, args.warmup, args.reps)
    r['unfused_over_fused_of_means'] = r['unfused']['mean'] / r['fused']['mean']
    rec['average_predict_eager'] = r
    fused.capture_graph(inputs)
    unfused.capture_graph(inputs)
    r = alternate({'fused': lambda: fused._predict_batch(inputs), 'unfused': lambda: unfused._predict_batch(inputs)},
                  dev, args.warmup, args.reps)
    r['unfused_over_fused_of_means'] = r['unfused']['mean'] / r['fused']['mean']
    rec['average_predict_graph'] = r

    Sa, Sb, ba, bb, n, hi, wi = run_lowres_scores(fused, inputs)
    out = torch.empty((n, 8 * hi, 8 * wi), dtype=torch.int64, device=dev)
    probs = [torch.empty((n, 8 * hi, 8 * wi, C), dtype=torch.float32, device=dev) for _ in range(2)]
    cm = torch.zeros((C, C), dtype=torch.int64, device=dev)

    def three_launches():
        ops.decoder_head_from_scores(Sa, ba, n, hi, wi, C, prob=probs[0])
        ops.decoder_head_from_scores(Sb, bb, n, hi, wi, C, prob=probs[1])
        return ops.average_fuse(probs)
    r = alternate({'fused_head_average': lambda: ops.fused_head_average(Sa, Sb, ba, bb, n, hi, wi, C, out=out),
                   'two_decoder_heads_and_average_fuse': three_launches,
                   'fused_head_average_count': lambda: ops.fused_head_average_count(Sa, Sb, ba, bb, n, hi, wi, C, test['labels'],
                                                                                    cm=cm)}, dev, args.warmup, 2 * args.reps)
    r['three_launches_over_head_of_means'] = r['two_decoder_heads_and_average_fuse']['mean'] / r['fused_head_average']['mean']
    rec['heads'] = r

    # ---- (b) the comparison flow against the per-model flows
    with tempfile.TemporaryDirectory() as tmp:
        weights = {}
        for m in prefixes:
            weights[m] = os.path.join(tmp, m + '.npz')
            np.savez(weights[m], **{k: v for k, v in fused.variables.items() if k.startswith(m + '/')})
        bayes_config = dict(common, prefixes=prefixes)
        dirichlet_config = dict(common, modalities=list(prefixes), sigma=1.0, delta=1e-2, beta=1e-2)
        all_config = dict(bayes_config, sigma=1.0, delta=1e-2, beta=1e-2)

        def per_model_flows():
            experiments.fit_and_evaluate_bayes_fusion(bayes_config, desc, measure, test, weights)
            experiments.fit_and_evaluate_dirichlet_fusion(dirichlet_config, desc, measure, test, weights)
            with get_model('average_fusion')(data_description=desc, **bayes_config) as net:
                experiments.import_weights_into_network(net, weights)
                net.score(test)
        r = alternate({'fit_and_evaluate_all_fusions': lambda: experiments.fit_and_evaluate_all_fusions(all_config, desc, measure,
                                                                                                        test, weights),
                       'per_model_flows': per_model_flows}, dev, 1, args.flow_reps, timer=wall_time)
        r['per_model_over_all_of_means'] = r['per_model_flows']['mean'] / r['fit_and_evaluate_all_fusions']['mean']
        rec['flows_wall_clock'] = r
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
