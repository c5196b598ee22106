#!/usr/bin/env python3
"""Cost of the expert-agreement table at 768x384, C = 12, 16 images, in one process:
  (a) `heads`: per mode (Bayes, Dirichlet, mean) and E = 2, 3, 4 the one ops.fused_head_multi_agreement launch beside
      - `materialised`: the launches it replaces (E decoder heads writing labels -- and `prob` where the fusion reads it --, the
        fusion launch, ops.agreement_table) and
      - `count_head`: ops.fused_head_multi_count at one parameter set with expert_cm, the closest existing kernel,
      on the same low-resolution scores of real trunks, alternated; the integers of the first two are compared first;
  (b) `score_agreement`: DirichletFusion.score_agreement of a three-expert model on 16 resident images against the same model
      with fused_head=False, alternated.
Device times by events around `--inner` back-to-back calls of a form (a) or one pass (b); mean / min / std over repetitions.
Prints one JSON line (profiles/agreement_bench.json)."""
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
SECTIONS = ('heads', 'score_agreement')


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
        sys.exit('agreement_bench.py needs a GPU')
    from modular_semantic_segmentation_amd import get_model, ops
    from modular_semantic_segmentation_amd.basic_fusion_model import device_tables, run_lowres_scores_multi
    from modular_semantic_segmentation_amd.bayes_mix import bayes_tables
    from modular_semantic_segmentation_amd.dirichlet_mix import dirichlet_tables
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

    def dirichlet(mods):
        params = {m: rng.uniform(0.5, 2.0, (C, C)) + 4.0 * np.eye(C) for m in mods}
        params['class_counts'] = rng.integers(100, 1000, C).astype(np.float64)
        return params
    rec = {}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            rec = json.loads(f.read())
    rec.update({'tool': 'agreement_bench', 'shape': [N, H, W], 'num_classes': C, 'reps': args.reps, 'inner': args.inner,
                'unit': 's'})

    if 'heads' in args.sections:
        four = get_model('average_fusion')(data_description=description(MODS), prefixes={m: m for m in MODS}, **common(MODS))
        scores, biases, n, hi, wi = run_lowres_scores_multi(four, inputs)
        label_maps = [torch.empty((n, 8 * hi, 8 * wi), dtype=torch.int64, device=dev) for _ in MODS]
        probs = [torch.empty((n, 8 * hi, 8 * wi, C), dtype=torch.float32, device=dev) for _ in MODS]
        rec['heads'] = {}
        for e in (2, 3, 4):
            mods = MODS[:e]
            mats = [np.asarray(rng.integers(1, 50, (C, C)) + 400 * np.eye(C, dtype=np.int64), np.float32).T for _ in mods]
            params = dirichlet(mods)
            S, b = scores[:e], biases[:e]
            for mode in MODES:
                if mode == 'bayes':
                    tables = dict(zip(('tab', 'logprior'), device_tables(dev, *bayes_tables(mats, 'data'))))
                elif mode == 'dirichlet':
                    tables = dict(zip(('tab', 'lognorm', 'logprior'), device_tables(dev, *dirichlet_tables(
                        [params[m].astype(np.float32) for m in mods], params['class_counts'].astype(np.float32), 'data', 1.0))))
                else:
                    tables = {}
                count_tables = {k: (v if (mode == 'bayes' and k == 'tab') else v[None].contiguous()) for k, v in tables.items()}
                table = torch.zeros((C, 1 << e, 2, 3), dtype=torch.int64, device=dev)
                table_m = torch.zeros_like(table)
                cm = torch.zeros((1, C, C), dtype=torch.int64, device=dev)
                expert_cm = torch.zeros((e, C, C), dtype=torch.int64, device=dev)

                def head(mode=mode, tables=tables, table=table):
                    return ops.fused_head_multi_agreement(S, b, n, hi, wi, C, mode, labels, table=table, **tables)

                def materialised(mode=mode, tables=tables, table=table_m):
                    for i in range(e):
                        ops.decoder_head_from_scores(S[i], b[i], n, hi, wi, C, label=label_maps[i],
                                                     prob=None if mode == 'bayes' else probs[i])
                    if mode == 'bayes':
                        fused = ops.bayes_fuse(label_maps[:e], tables['tab'], tables['logprior'])[0]
                    elif mode == 'dirichlet':
                        fused = ops.dirichlet_fuse(probs[:e], tables['tab'], tables['lognorm'], tables['logprior'])[0]
                    else:
                        fused = ops.average_fuse(probs[:e])
                    return ops.agreement_table(labels, label_maps[:e], fused, C, table=table)

                def count_head(mode=mode, tables=count_tables):
                    return ops.fused_head_multi_count(S, b, n, hi, wi, C, mode, labels, cm=cm, expert_cm=expert_cm, **tables)
                head()
                materialised()
                assert torch.equal(table, table_m), (e, mode)
                r = alternate({'agreement_head': head, 'materialised': materialised, 'count_head': count_head}, dev,
                              args.warmup, args.reps, args.inner)
                r['materialised_launch_count'] = e + 2
                r['materialised_over_agreement_of_means'] = r['materialised']['mean'] / r['agreement_head']['mean']
                r['count_head_over_agreement_of_means'] = r['count_head']['mean'] / r['agreement_head']['mean']
                rec['heads']['%s_e%d' % (mode, e)] = r
        del four

    if 'score_agreement' in args.sections:
        mods = MODS[:3]
        data = {k: host[k] for k in mods + ('labels',)}
        config = dict(common(mods), modalities=list(mods), dirichlet_params=dirichlet(mods), sigma=1.0, delta=1e-2, beta=1e-2)
        fused = get_model('dirichlet_fusion')(data_description=description(mods), **config)
        generic = get_model('dirichlet_fusion')(data_description=description(mods), **dict(config, fused_head=False))
        generic.variables.update(fused.variables)
        generic._variables_changed()
        assert np.array_equal(fused.score_agreement(data)[1], generic.score_agreement(data)[1])
        r = alternate({'fused': lambda: fused.score_agreement(data), 'generic': lambda: generic.score_agreement(data)}, dev,
                      args.warmup, args.reps)
        r['generic_over_fused_of_means'] = r['generic']['mean'] / r['fused']['mean']
        rec['dirichlet_fusion_score_agreement'] = r
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
