#!/usr/bin/env python3
"""Cost of the confidence maps at 768x384, C = 12, 16 images, in one process:
  (a) `heads`: per mode (Bayes, Dirichlet, mean) and E = 2, 3, 4, on the same low-resolution scores of real trunks, alternated:
      `confidence_2` the one ops.fused_head_multi_confidence launch writing label + confidence, `confidence_4` the same launch
      with all four maps, `materialised` the launches it replaces -- E decoder heads writing probability maps (Bayes: label
      maps), the fusion launch with its score output (the mean: the averaged probabilities) and ops.confidence_map with label +
      confidence -- and `label_only` ops.fused_head_multi, which shows what the confidence costs on top of a label.  The maps of
      the first and third are compared first;
  (b) `predict_confidence`: DirichletFusion.predict_confidence of a three-expert model on 16 resident images against predict()
      and against predict(output_attr='fused_score'), end to end (results fetched to the host), alternated.
Device times by events around `--inner` back-to-back calls of a form (a) or one pass (b); mean / min / std over repetitions.
Prints one JSON line (profiles/confidence_bench.json)."""
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
ALL = ('label', 'confidence', 'entropy', 'margin')
SECTIONS = ('heads', 'predict_confidence')


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
        sys.exit('confidence_bench.py needs a GPU')
    from modular_semantic_segmentation_amd import get_model, ops
    from modular_semantic_segmentation_amd.basic_fusion_model import device_tables, run_lowres_scores_multi
    from modular_semantic_segmentation_amd.bayes_mix import bayes_tables
    from modular_semantic_segmentation_amd.dirichlet_mix import dirichlet_tables
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    rng = np.random.default_rng(0)
    host = {m: rng.integers(0, 256 if m in ('rgb', 'gray') else 65536, (N, H, W, CHANNELS[m])).astype(np.float32) for m in MODS}
    inputs = {m: torch.from_numpy(host[m]).to(dev) for m in MODS}

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
    rec.update({'tool': 'confidence_bench', 'shape': [N, H, W], 'num_classes': C, 'reps': args.reps, 'inner': args.inner,
                'unit': 's'})

    if 'heads' in args.sections:
        four = get_model('average_fusion')(data_description=description(MODS), prefixes={m: m for m in MODS}, **common(MODS))
        scores, biases, n, hi, wi = run_lowres_scores_multi(four, inputs)
        shape = (n, 8 * hi, 8 * wi)
        label_maps = [torch.empty(shape, dtype=torch.int64, device=dev) for _ in MODS]
        probs = [torch.empty(shape + (C,), dtype=torch.float32, device=dev) for _ in MODS]
        outs = [{k: torch.empty(shape, dtype=ops.CONFIDENCE_MAPS[k], device=dev) for k in ALL} for _ in range(2)]
        fused_label = torch.empty(shape, dtype=torch.int64, device=dev)
        rec['heads'] = {}
        for e in (2, 3, 4):
            mods = MODS[:e]
            mats = [np.asarray(rng.integers(1, 50, (C, C)) + 400 * np.eye(C, dtype=np.int64), np.float32).T for _ in mods]
            params = dirichlet(mods)
            S, b = scores[:e], biases[:e]
            divisor = torch.tensor(float(e), device=dev)
            for mode in MODES:
                if mode == 'bayes':
                    tables = dict(zip(('tab', 'logprior'), device_tables(dev, *bayes_tables(mats, 'data'))))
                elif mode == 'dirichlet':
                    tables = dict(zip(('tab', 'lognorm', 'logprior'), device_tables(dev, *dirichlet_tables(
                        [params[m].astype(np.float32) for m in mods], params['class_counts'].astype(np.float32), 'data', 1.0))))
                else:
                    tables = {}

                def head(want, mode=mode, tables=tables):
                    return ops.fused_head_multi_confidence(S, b, n, hi, wi, C, mode, 1.5, want=want, out=outs[0], **tables)

                def materialised(mode=mode, tables=tables):
                    for i in range(e):
                        ops.decoder_head_from_scores(S[i], b[i], n, hi, wi, C, label=label_maps[i] if mode == 'bayes' else None,
                                                     prob=None if mode == 'bayes' else probs[i])
                    if mode == 'bayes':
                        values, kind = ops.bayes_fuse(label_maps[:e], tables['tab'], tables['logprior'], want_score=True)[1], 0
                    elif mode == 'dirichlet':
                        values, kind = ops.dirichlet_fuse(probs[:e], tables['tab'], tables['lognorm'], tables['logprior'],
                                                          want_score=True)[1], 0
                    else:
                        total = probs[0]
                        for p in probs[1:e]:
                            total = total + p
                        values, kind = total / divisor, 1
                    return ops.confidence_map(values, 1.5, kind=kind, want=ALL[:2], out=outs[1])

                def label_only(mode=mode, tables=tables):
                    return ops.fused_head_multi(S, b, n, hi, wi, C, mode, out=fused_label, **tables)
                head(ALL[:2])
                materialised()
                label_only()
                assert torch.equal(outs[0]['label'], outs[1]['label']) and torch.equal(outs[0]['label'], fused_label), (e, mode)
                differ = float((outs[0]['confidence'] - outs[1]['confidence']).abs().max())
                r = alternate({'confidence_2': lambda: head(ALL[:2]), 'confidence_4': lambda: head(ALL),
                               'materialised': materialised, 'label_only': label_only}, dev, args.warmup, args.reps, args.inner)
                r['max_confidence_difference'] = differ
                r['materialised_over_confidence_2_of_means'] = r['materialised']['mean'] / r['confidence_2']['mean']
                r['confidence_2_over_label_only_of_means'] = r['confidence_2']['mean'] / r['label_only']['mean']
                rec['heads']['%s_e%d' % (mode, e)] = r
        del four

    if 'predict_confidence' in args.sections:
        mods = MODS[:3]
        data = {k: host[k] for k in mods}
        config = dict(common(mods), modalities=list(mods), dirichlet_params=dirichlet(mods), sigma=1.0, delta=1e-2, beta=1e-2)
        net = get_model('dirichlet_fusion')(data_description=description(mods), **config)
        assert np.array_equal(net.predict_confidence(data)['label'], net.predict(data))
        r = alternate({'predict_confidence': lambda: net.predict_confidence(data),
                       'predict_confidence_4': lambda: net.predict_confidence(data, outputs=ALL[1:]),
                       'predict': lambda: net.predict(data),
                       'predict_fused_score': lambda: net.predict(data, output_attr='fused_score')}, dev, args.warmup, args.reps)
        r['predict_confidence_over_predict_of_means'] = r['predict_confidence']['mean'] / r['predict']['mean']
        r['predict_fused_score_over_predict_confidence_of_means'] = r['predict_fused_score']['mean'] / r['predict_confidence']['mean']
        rec['dirichlet_fusion_predict_confidence'] = r
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
