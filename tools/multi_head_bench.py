#!/usr/bin/env python3
"""Cost of the fused head for three and four experts at 768x384, C = 12, 16 images, in one process:
  (a) per mode (Bayes, Dirichlet, mean) and E = 3, 4: the one ops.fused_head_multi launch beside the E + 1 launches it replaces
      (E decoder heads writing labels / `prob`, then bayes_fuse / dirichlet_fuse / average_fuse) on the same low-resolution
      scores of real trunks, alternated; the labels of the two are compared first;
  (b) predict of a three-expert bayes_fusion / dirichlet_fusion / average_fusion on 16 resident images, the fused default
      path against the same model with fused_head=False (the route every model with more than two experts took before the
      head existed, unchanged), alternated, eager and replayed from a captured graph.
Device times by events around `--inner` back-to-back calls of a form (a) or one step (b); mean / min / std over repetitions.
Prints one JSON line; --out also writes it (profiles/multi_head_bench.json)."""
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
    ap.add_argument('--inner', type=int, default=20, help='back-to-back calls per timed window of the head forms')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None, help='also write the JSON record here')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('multi_head_bench.py needs a GPU')
    from modular_semantic_segmentation_amd import get_model, ops
    from modular_semantic_segmentation_amd.basic_fusion_model import device_tables, run_lowres_scores_multi
    from modular_semantic_segmentation_amd.bayes_mix import bayes_tables
    from modular_semantic_segmentation_amd.dirichlet_mix import dirichlet_tables
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    rng = np.random.default_rng(0)
    inputs = {m: torch.from_numpy(rng.integers(0, 256 if m in ('rgb', 'gray') else 65536, (N, H, W, CHANNELS[m]))
                                  .astype(np.float32)).to(dev) for m in MODS}

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
    rec = {'tool': 'multi_head_bench', 'shape': [N, H, W], 'num_classes': C, 'reps': args.reps, 'inner': args.inner, 'unit': 's'}

    # ---- (a) the head launch beside the launches it replaces, on the scores of four real trunks
    four = get_model('average_fusion')(data_description=description(MODS), prefixes={m: m for m in MODS}, **common(MODS))
    scores, biases, n, hi, wi = run_lowres_scores_multi(four, inputs)
    out = torch.empty((n, 8 * hi, 8 * wi), dtype=torch.int64, device=dev)
    labels = [torch.empty((n, 8 * hi, 8 * wi), dtype=torch.int64, device=dev) for _ in MODS]
    probs = [torch.empty((n, 8 * hi, 8 * wi, C), dtype=torch.float32, device=dev) for _ in MODS]
    rec['heads'] = {}
    for e in (3, 4):
        mods = MODS[:e]
        loglik, logprior_b = device_tables(dev, *bayes_tables([np.asarray(m, np.float32).T for m in confusion(mods).values()]))
        params = dirichlet(mods)
        am1, lognorm, logprior_d = device_tables(dev, *dirichlet_tables(
            [params[m].astype(np.float32) for m in mods], params['class_counts'].astype(np.float32), 'data', 1.0))
        S, b = scores[:e], biases[:e]
        tables = {'bayes': dict(tab=loglik, logprior=logprior_b),
                  'dirichlet': dict(tab=am1, lognorm=lognorm, logprior=logprior_d), 'mean': {}}

        def unfused(mode):
            for i in range(e):
                if mode == 'bayes':
                    ops.decoder_head_from_scores(S[i], b[i], n, hi, wi, C, label=labels[i])
                else:
                    ops.decoder_head_from_scores(S[i], b[i], n, hi, wi, C, prob=probs[i])
            if mode == 'bayes':
                return ops.bayes_fuse(labels[:e], loglik, logprior_b)[0]
            if mode == 'dirichlet':
                return ops.dirichlet_fuse(probs[:e], am1, lognorm, logprior_d)[0]
            return ops.average_fuse(probs[:e])
        for mode in MODES:
            def head(mode=mode):
                return ops.fused_head_multi(S, b, n, hi, wi, C, mode, out=out, **tables[mode])
            assert torch.equal(head(), unfused(mode)), (e, mode)
            r = alternate({'fused_head_multi': head, 'decoder_heads_and_fusion': lambda mode=mode: unfused(mode)}, dev,
                          args.warmup, args.reps, args.inner)
            r['launches_replaced'] = e + 1
            r['replaced_over_head_of_means'] = r['decoder_heads_and_fusion']['mean'] / r['fused_head_multi']['mean']
            rec['heads']['%s_e%d' % (mode, e)] = r
    del four

    # ---- (b) predict of the three-expert models, fused against fused_head=False
    mods = MODS[:3]
    batch = {m: inputs[m] for m in mods}
    extra = {'bayes_fusion': dict(prefixes={m: m for m in mods}, confusion_matrices=confusion(mods)),
             'dirichlet_fusion': dict(modalities=list(mods), dirichlet_params=dirichlet(mods), sigma=1.0, delta=1e-2, beta=1e-2),
             'average_fusion': dict(prefixes={m: m for m in mods})}
    for kind, config in extra.items():
        fused = get_model(kind)(data_description=description(mods), **dict(common(mods), **config))
        unfused_net = get_model(kind)(data_description=description(mods), fused_head=False, **dict(common(mods), **config))
        unfused_net.variables.update(fused.variables)
        unfused_net._variables_changed()
        assert np.array_equal(fused.predict(batch), unfused_net.predict(batch)), kind
        r = alternate({'fused': lambda: fused._predict_batch_impl(batch), 'unfused': lambda: unfused_net._predict_batch_impl(batch)},
                      dev, args.warmup, args.reps)
        r['unfused_over_fused_of_means'] = r['unfused']['mean'] / r['fused']['mean']
        rec['%s_predict_eager' % kind] = r
        fused.capture_graph(batch)
        unfused_net.capture_graph(batch)
        r = alternate({'fused': lambda: fused._predict_batch(batch), 'unfused': lambda: unfused_net._predict_batch(batch)},
                      dev, args.warmup, args.reps)
        r['unfused_over_fused_of_means'] = r['unfused']['mean'] / r['fused']['mean']
        r['images_per_s_fused'] = N / r['fused']['mean']
        r['images_per_s_unfused'] = N / r['unfused']['mean']
        rec['%s_predict_graph' % kind] = r
        del fused, unfused_net
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
