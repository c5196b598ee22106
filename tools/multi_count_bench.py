#!/usr/bin/env python3
"""Cost of the counting head for three and four experts at 768x384, C = 12, 16 images, in one process:
  (a) `heads`: per mode (Bayes, Dirichlet, mean), E = 3, 4 and G = 1, 4, 16 parameter sets (mean: 1): the one
      ops.fused_head_multi_count launch beside the launches the generic route makes for the same counts (E decoder heads writing
      labels / `prob`, then per set a fusion launch and a confusion launch) on the same low-resolution scores of real trunks,
      alternated; the integers of the two are compared first;
  (b) `score_grid`: DirichletFusion.score_grid (sigma x class_prior, four sets) and BayesFusion.score_grid (three priors) of a
      three-expert model on 16 resident images, the counting head against the same model with fused_head=False (the generic
      route, what every model with more than two experts ran before the head existed), alternated;
  (c) `score_all`: FusionComparison.score_all of three experts, the same two routes.
Device times by events around `--inner` back-to-back calls of a form (a) or one pass (b, c); mean / min / std over repetitions.
--sections picks the parts of one call (a part per process keeps each run short); the record of --out is read back first, so
that several calls fill one file.  Prints one JSON line (profiles/multi_count_bench.json)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
C, U, H, W, N = 12, 64, 384, 768, 16
MODS = ('rgb', 'depth', 'ir', 'gray')
CHANNELS = {'rgb': 3, 'depth': 1, 'ir': 1, 'gray': 1}
MODES = ('bayes', 'dirichlet', 'mean')
POINTS = (1, 4, 16)
SECTIONS = ('heads', 'score_grid', 'score_all')


def event_time(fn, dev, inner=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) * 1e-3 / inner


def stats(v):
    return {'mean': float(np.mean(v)), 'min': float(np.min(v)), 'std': float(np.std(v))}


def alternate(forms, dev, warmup, reps, inner=1):
    for _ in range(warmup):
        for f in forms.values():
            f()
    times = {k: [] for k in forms}
    for _ in range(reps):
        for k, f in forms.items():
            times[k].append(event_time(f, dev, inner))
    return {k: stats(v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--inner', type=int, default=10, help='back-to-back calls per timed window of the head forms')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--sections', nargs='+', choices=SECTIONS, default=list(SECTIONS))
    ap.add_argument('--out', default=None, help='also write the JSON record here (merged into what the file holds)')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('multi_count_bench.py needs a GPU')
    from modular_semantic_segmentation_amd import get_model, ops
    from modular_semantic_segmentation_amd.basic_fusion_model import device_tables, run_lowres_scores_multi
    from modular_semantic_segmentation_amd.bayes_mix import bayes_tables
    from modular_semantic_segmentation_amd.dirichlet_mix import dirichlet_tables
    from modular_semantic_segmentation_amd.fusion_comparison import FusionComparison
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    rng = np.random.default_rng(0)
    host = {m: rng.integers(0, 256 if m in ('rgb', 'gray') else 65536, (N, H, W, CHANNELS[m])).astype(np.float32) for m in MODS}
    host['labels'] = rng.integers(-1, C, (N, H, W)).astype(np.int32)
    inputs = {m: torch.from_numpy(host[m]).to(dev) for m in MODS}
    labels = torch.from_numpy(host['labels']).to(dev)

    def description(mods):
        return (dict({m: 'float32' for m in mods}, labels='int32'),
                dict({m: (None, None, CHANNELS[m]) for m in mods}, labels=(None, None)), C)

    def common(mods):
        return dict(num_units=U, num_channels={m: CHANNELS[m] for m in mods}, expert_model='fcn', batchsize=N, class_prior='data',
                    seed=1, device=str(dev))

    def confusion(mods):
        return {m: rng.integers(1, 50, (C, C)) + 400 * np.eye(C, dtype=np.int64) for m in mods}

    def dirichlet(mods):
        params = {m: rng.uniform(0.5, 2.0, (C, C)) + 4.0 * np.eye(C) for m in mods}
        params['class_counts'] = rng.integers(100, 1000, C).astype(np.float64)
        return params
    rec = {}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            rec = json.loads(f.read())
    rec.update({'tool': 'multi_count_bench', 'shape': [N, H, W], 'num_classes': C, 'reps': args.reps, 'inner': args.inner,
                'unit': 's'})

    # ---- (a) the counting launch beside the launches of the generic route, on the scores of four real trunks
    if 'heads' in args.sections:
        four = get_model('average_fusion')(data_description=description(MODS), prefixes={m: m for m in MODS}, **common(MODS))
        scores, biases, n, hi, wi = run_lowres_scores_multi(four, inputs)
        label_maps = [torch.empty((n, 8 * hi, 8 * wi), dtype=torch.int64, device=dev) for _ in MODS]
        probs = [torch.empty((n, 8 * hi, 8 * wi, C), dtype=torch.float32, device=dev) for _ in MODS]
        rec['heads'] = {}
        for e in (3, 4):
            mods = MODS[:e]
            mats = [np.asarray(m, np.float32).T for m in confusion(mods).values()]
            params = dirichlet(mods)
            S, b = scores[:e], biases[:e]
            for mode in MODES:
                for G in ((1,) if mode == 'mean' else POINTS):
                    priors = ['data'] + [float(p) for p in np.linspace(0.1, 0.9, G - 1)]
                    if mode == 'bayes':
                        loglik = device_tables(dev, bayes_tables(mats, 'data')[0])[0]
                        logprior = torch.stack([device_tables(dev, bayes_tables(mats, p)[1])[0] for p in priors]).contiguous()
                        tables = dict(tab=loglik, logprior=logprior)
                    elif mode == 'dirichlet':
                        points = [device_tables(dev, *dirichlet_tables(
                            [params[m].astype(np.float32) for m in mods], params['class_counts'].astype(np.float32), 'data',
                            float(sigma))) for sigma in np.geomspace(0.2, 5.0, G)]
                        tables = dict(zip(('tab', 'lognorm', 'logprior'),
                                          (torch.stack([p[i] for p in points]).contiguous() for i in range(3))))
                    else:
                        tables = {}
                    cm = torch.zeros((G, C, C), dtype=torch.int64, device=dev)
                    cm_generic = torch.zeros((G, C, C), dtype=torch.int64, device=dev)

                    def head(mode=mode, tables=tables, cm=cm):
                        return ops.fused_head_multi_count(S, b, n, hi, wi, C, mode, labels, cm=cm, **tables)

                    def generic(mode=mode, tables=tables, cm=cm_generic, G=G):
                        for i in range(e):
                            if mode == 'bayes':
                                ops.decoder_head_from_scores(S[i], b[i], n, hi, wi, C, label=label_maps[i])
                            else:
                                ops.decoder_head_from_scores(S[i], b[i], n, hi, wi, C, prob=probs[i])
                        for g in range(G):
                            if mode == 'bayes':
                                fused = ops.bayes_fuse(label_maps[:e], tables['tab'], tables['logprior'][g])[0]
                            elif mode == 'dirichlet':
                                fused = ops.dirichlet_fuse(probs[:e], tables['tab'][g], tables['lognorm'][g],
                                                           tables['logprior'][g])[0]
                            else:
                                fused = ops.average_fuse(probs[:e])
                            ops.confusion_matrix(labels, fused.contiguous(), cm[g])
                    head()
                    generic()
                    assert torch.equal(cm, cm_generic), (e, mode, G)
                    r = alternate({'fused_head_multi_count': head, 'generic_launches': generic}, dev, args.warmup, args.reps,
                                  args.inner)
                    r['generic_launch_count'] = e + 2 * G
                    r['generic_over_count_of_means'] = r['generic_launches']['mean'] / r['fused_head_multi_count']['mean']
                    rec['heads']['%s_e%d_g%d' % (mode, e, G)] = r
        del four

    # ---- (b), (c) the evaluation flows of three-expert models, the counting head against fused_head=False
    mods = MODS[:3]
    data = {k: host[k] for k in mods + ('labels',)}

    def pair(build):
        fused, generic = build(), build(fused_head=False)
        generic.variables.update(fused.variables)
        generic._variables_changed()
        return fused, generic

    def record(key, fused_fn, generic_fn, same):
        assert same(fused_fn(), generic_fn()), key
        r = alternate({'fused': fused_fn, 'generic': generic_fn}, dev, args.warmup, args.reps)
        r['generic_over_fused_of_means'] = r['generic']['mean'] / r['fused']['mean']
        rec[key] = r

    def same_grid(a, b):
        return all(np.array_equal(x[2], y[2]) for x, y in zip(a, b))
    if 'score_grid' in args.sections:
        grids = {'dirichlet_fusion': {'sigma': [0.5, 1.0], 'class_prior': ['data', 'uniform']},
                 'bayes_fusion': {'class_prior': ['data', 'uniform', 0.5]}}
        extra = {'bayes_fusion': dict(prefixes={m: m for m in mods}, confusion_matrices=confusion(mods)),
                 'dirichlet_fusion': dict(modalities=list(mods), dirichlet_params=dirichlet(mods), sigma=1.0, delta=1e-2,
                                          beta=1e-2)}
        for kind, config in extra.items():
            fused, generic = pair(lambda **kw: get_model(kind)(data_description=description(mods),
                                                               **dict(common(mods), **config, **kw)))
            record('%s_score_grid' % kind, lambda: fused.score_grid(data, grids[kind]),
                   lambda: generic.score_grid(data, grids[kind]), same_grid)
            del fused, generic
    if 'score_all' in args.sections:
        cms, params = confusion(mods), dirichlet(mods)
        fused, generic = pair(lambda **kw: FusionComparison(
            data_description=description(mods), prefixes={m: m for m in mods}, confusion_matrices=cms, dirichlet_params=params,
            sigma=1.0, delta=1e-2, beta=1e-2, **dict(common(mods), **kw)))
        record('comparison_score_all', lambda: fused.score_all(data), lambda: generic.score_all(data),
               lambda a, b: all(np.array_equal(a[k][1], b[k][1]) for k in a))
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
