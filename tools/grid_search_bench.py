#!/usr/bin/env python3
"""Cost of a grid search over the fusion parameters at 16 resident images of 768x384 RGB-D, C = 12, for G = 1 / 4 / 16 grid
points and both fusion models, two routes alternated in one process:
  score_grid   one pass of the experts, every grid point fused and counted by the grid-scoring head;
  score_calls  G calls of score() with the config changed (and the tables rebuilt) between them: what a user had to do before.
Device times by events around each route (mean / min / std over repetitions; the host work between the launches of a route is
inside its interval, as it is for a user).  The new Dirichlet head at G = 1 is timed beside xv_fused_head_fwd +
xv_confusion_matrix on the same low-resolution scores, and the joint histogram beside the Bayes form of the same pair.
Prints one JSON line; --out also writes it (profiles/grid_search_bench.json)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
C, U, H, W, N = 12, 64, 384, 768, 16
SIGMAS = [0.25, 0.5, 1.0, 2.0]
PRIORS = ['data', 'uniform', 0.3, 0.7]
BAYES_PRIORS = ['data', 'uniform'] + [round(0.05 + 0.065 * i, 3) for i in range(14)]


def event_time(fn, dev):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) * 1e-3


def stats(v):
    return {'mean': float(np.mean(v)), 'min': float(np.min(v)), 'std': float(np.std(v))}


def alternate(forms, dev, warmup, reps):
    for _ in range(warmup):
        for f in forms.values():
            f()
    times = {k: [] for k in forms}
    for _ in range(reps):
        for k, f in forms.items():
            times[k].append(event_time(f, dev))
    return {k: stats(v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None, help='also write the JSON record here')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('grid_search_bench.py needs a GPU')
    from modular_semantic_segmentation_amd import get_model, ops
    from modular_semantic_segmentation_amd.basic_fusion_model import parameter_combinations, run_lowres_scores
    from modular_semantic_segmentation_amd.bayes_mix import bayes_tables
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    rng = np.random.default_rng(0)
    data = {'rgb': torch.from_numpy(rng.integers(0, 256, (N, H, W, 3)).astype(np.float32)).to(dev),
            'depth': torch.from_numpy(rng.integers(0, 65536, (N, H, W, 1)).astype(np.float32)).to(dev),
            'labels': torch.from_numpy(rng.integers(-1, C, (N, H, W)).astype(np.int32)).to(dev)}
    desc = ({'labels': 'int32', 'rgb': 'float32', 'depth': 'float32'},
            {'labels': (None, None), 'rgb': (None, None, 3), 'depth': (None, None, 1)}, C)
    common = dict(data_description=desc, num_units=U, num_channels={'rgb': 3, 'depth': 1}, expert_model='fcn', batchsize=N,
                  class_prior='data', seed=1, device=str(dev))
    cms = {m: rng.integers(1, 1000, (C, C)) + 20000 * np.eye(C, dtype=np.int64) for m in ('rgb', 'depth')}
    params = {'rgb': rng.uniform(0.5, 4.0, (C, C)), 'depth': rng.uniform(0.5, 4.0, (C, C)), 'class_counts': cms['depth'].sum(1)}
    dirichlet = get_model('dirichlet_fusion')(dirichlet_params=params, modalities=['rgb', 'depth'], sigma=1.0, delta=1e-2,
                                              beta=1e-2, **common)
    bayes = get_model('bayes_fusion')(confusion_matrices=cms, prefixes={'rgb': 'rgb', 'depth': 'depth'}, **common)

    def dirichlet_calls(search):
        for config in parameter_combinations(search, dirichlet.config):
            dirichlet.config.update({k: config[k] for k in search})
            dirichlet._initialize_graph()                 # the tables of this point, as the constructor builds them
            dirichlet.score(data)

    def bayes_calls(search):
        mats = [bayes.confusion_matrices[m] for m in bayes.modalities]
        for prior in search['class_prior']:
            bayes.config['class_prior'] = prior           # the tables alone: a rebuilt model would re-create its engines too
            loglik, logprior = bayes_tables(mats, prior)
            bayes.loglik, bayes.logprior = torch.from_numpy(loglik).to(dev), torch.from_numpy(logprior).to(dev)
            bayes.score(data)

    rec = {'tool': 'grid_search_bench', 'shape': [N, H, W], 'num_classes': C, 'reps': args.reps, 'unit': 's', 'dirichlet': {},
           'bayes': {}}
    searches = {1: {'sigma': SIGMAS[2:3], 'class_prior': PRIORS[:1]}, 4: {'sigma': SIGMAS[:2], 'class_prior': PRIORS[:2]},
                16: {'sigma': SIGMAS, 'class_prior': PRIORS}}
    for G, search in searches.items():
        r = alternate({'score_grid': lambda: dirichlet.score_grid(data, search), 'score_calls': lambda: dirichlet_calls(search)},
                      dev, args.warmup, args.reps)
        r['speedup_of_means'] = r['score_calls']['mean'] / r['score_grid']['mean']
        rec['dirichlet'][str(G)] = r
        bsearch = {'class_prior': BAYES_PRIORS[:G]}
        r = alternate({'score_grid': lambda: bayes.score_grid(data, bsearch), 'score_calls': lambda: bayes_calls(bsearch)},
                      dev, args.warmup, args.reps)
        r['speedup_of_means'] = r['score_calls']['mean'] / r['score_grid']['mean']
        rec['bayes'][str(G)] = r
    # the heads alone, on one batch's low-resolution scores
    Sa, Sb, ba, bb, n, hi, wi = run_lowres_scores(dirichlet, data)
    labels = data['labels']
    am1, lognorm, logprior = dirichlet.am1, dirichlet.lognorm, dirichlet.logprior
    cm1 = torch.zeros((1, C, C), dtype=torch.int64, device=dev)
    cm = torch.zeros((C, C), dtype=torch.int64, device=dev)
    hist = torch.zeros((C, C, C), dtype=torch.int64, device=dev)
    pred = torch.empty((n, 8 * hi, 8 * wi), dtype=torch.int64, device=dev)

    def head_and_count(tab, lp, ln=None):
        ops.fused_head(Sa, Sb, ba, bb, n, hi, wi, C, tab, lp, lognorm=ln, out=pred)
        ops.confusion_matrix(labels, pred, cm)
    tabs16 = [t[None].repeat(16, *([1] * t.dim())).contiguous() for t in (am1, lognorm, logprior)]
    cm16 = torch.zeros((16, C, C), dtype=torch.int64, device=dev)
    rec['heads'] = alternate({
        'grid_score_1_point': lambda: ops.fused_head_grid_score(Sa, Sb, ba, bb, n, hi, wi, C, am1[None], lognorm[None],
                                                                logprior[None], labels, cm=cm1),
        'grid_score_16_points': lambda: ops.fused_head_grid_score(Sa, Sb, ba, bb, n, hi, wi, C, *tabs16, labels, cm=cm16),
        'fused_head_dirichlet_and_confusion': lambda: head_and_count(am1, logprior, lognorm),
        'joint_hist': lambda: ops.fused_head_joint_hist(Sa, Sb, ba, bb, n, hi, wi, C, labels, hist=hist),
        'fused_head_bayes_and_confusion': lambda: head_and_count(bayes.loglik, bayes.logprior)}, dev, args.warmup, 2 * args.reps)
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
