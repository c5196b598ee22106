#!/usr/bin/env python3
"""Cost of the IBCC fusion's label-tuple heads at 768x384, C = 12, 16 images, E = 2 / 3 / 4, in one process:
  (a) `hist`: the one ops.fused_head_multi_tuple_hist launch beside what it replaces -- E decoder heads writing label maps,
      the tuple index and a torch.bincount over it -- on the same low-resolution scores of real trunks, alternated; the
      integers are compared first;
  (b) `lut`: ops.fused_head_multi_lut beside ops.fused_head_multi in Bayes mode (the closest existing head: the same
      per-expert work, its decision from log-likelihood sums or a table it builds itself), alternated;
  (c) `end_to_end`: IbccFusion.adapt() + score() on 16 resident images against the same model with fused_head=False,
      alternated; the integers are compared first.
Device times by events around `--inner` back-to-back calls of a form (a, b: 100 by default, windows of 4 ms and more) or one
pass (c); mean / min / std over repetitions.  Prints one JSON line (profiles/ibcc_bench.json)."""
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
SECTIONS = ('hist', 'lut', 'end_to_end')


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
    ap.add_argument('--inner', type=int, default=100, help='back-to-back calls per timed window of the head forms')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--sections', nargs='+', choices=SECTIONS, default=list(SECTIONS))
    ap.add_argument('--experts', nargs='+', type=int, choices=(2, 3, 4), default=[2, 3, 4])
    ap.add_argument('--out', default=None, help='also write the JSON record here (merged into what the file holds)')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('ibcc_bench.py needs a GPU')
    from modular_semantic_segmentation_amd import get_model, ops
    from modular_semantic_segmentation_amd.basic_fusion_model import device_tables, run_lowres_scores_multi
    from modular_semantic_segmentation_amd.bayes_mix import bayes_tables
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
        return dict(num_units=U, num_channels={m: CHANNELS[m] for m in mods}, expert_model='fcn', batchsize=N, seed=1,
                    device=str(dev), prefixes={m: m for m in mods})

    def matrices(mods):
        return {m: rng.integers(1, 50, (C, C)) + 400 * np.eye(C, dtype=np.int64) for m in mods}
    rec = {}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            rec = json.loads(f.read())
    rec.update({'tool': 'ibcc_bench', 'shape': [N, H, W], 'num_classes': C, 'reps': args.reps, 'inner': args.inner, 'unit': 's'})

    if 'hist' in args.sections or 'lut' in args.sections:
        four = get_model('average_fusion')(data_description=description(MODS), **common(MODS))
        scores, biases, n, hi, wi = run_lowres_scores_multi(four, inputs)
        label_maps = [torch.empty((n, 8 * hi, 8 * wi), dtype=torch.int64, device=dev) for _ in MODS]
        for e in args.experts:
            S, b, T = scores[:e], biases[:e], C ** e
            if 'hist' in args.sections:
                hist = torch.zeros(T, dtype=torch.int64, device=dev)
                hist_m = torch.zeros(T, dtype=torch.int64, device=dev)

                def head(hist=hist):
                    return ops.fused_head_multi_tuple_hist(S, b, n, hi, wi, C, hist=hist)

                def materialised(hist=hist_m):
                    t = None
                    for i in range(e):
                        ops.decoder_head_from_scores(S[i], b[i], n, hi, wi, C, label=label_maps[i])
                        t = label_maps[i] if t is None else t * C + label_maps[i]
                    hist += torch.bincount(t.reshape(-1), minlength=T)
                    return hist
                head()
                materialised()
                assert torch.equal(hist, hist_m), e
                r = alternate({'tuple_hist_head': head, 'materialised': materialised}, dev, args.warmup, args.reps, args.inner)
                r['materialised_over_head_of_means'] = r['materialised']['mean'] / r['tuple_hist_head']['mean']
                rec.setdefault('hist', {})['e%d' % e] = r
            if 'lut' in args.sections:
                mats = [np.asarray(m, np.float32).T for m in matrices(MODS[:e]).values()]
                tab, logprior = device_tables(dev, *bayes_tables(mats, 'data'))
                lut = torch.from_numpy(rng.integers(0, C, T).astype(np.uint8)).to(dev)
                out = torch.empty((n, 8 * hi, 8 * wi), dtype=torch.int64, device=dev)
                cm = torch.zeros((C, C), dtype=torch.int64, device=dev)
                cm_b = torch.zeros((1, C, C), dtype=torch.int64, device=dev)
                r = alternate({
                    'lut_head': lambda: ops.fused_head_multi_lut(S, b, n, hi, wi, C, lut, out=out),
                    'bayes_head': lambda: ops.fused_head_multi(S, b, n, hi, wi, C, 'bayes', tab=tab, logprior=logprior, out=out),
                    'lut_count_head': lambda: ops.fused_head_multi_lut_count(S, b, n, hi, wi, C, lut, labels, cm=cm),
                    'bayes_count_head': lambda: ops.fused_head_multi_count(S, b, n, hi, wi, C, 'bayes', labels, tab=tab,
                                                                           logprior=logprior[None].contiguous(), cm=cm_b),
                }, dev, args.warmup, args.reps, args.inner)
                r['bayes_over_lut_of_means'] = r['bayes_head']['mean'] / r['lut_head']['mean']
                r['bayes_count_over_lut_count_of_means'] = r['bayes_count_head']['mean'] / r['lut_count_head']['mean']
                rec.setdefault('lut', {})['e%d' % e] = r
        del four

    if 'end_to_end' in args.sections:
        for e in args.experts:
            mods = MODS[:e]
            data = {k: host[k] for k in mods + ('labels',)}
            config = dict(common(mods), confusion_matrices=matrices(mods), prior_strength=20.0)
            fused = get_model('ibcc_fusion')(data_description=description(mods), **config)
            generic = get_model('ibcc_fusion')(data_description=description(mods), **dict(config, fused_head=False))
            generic.variables.update(fused.variables)
            generic._variables_changed()

            def run(net):
                net.adapt(data)
                return net.score(data)[1]
            assert np.array_equal(run(fused), run(generic)), e
            r = alternate({'fused': lambda: run(fused), 'generic': lambda: run(generic)}, dev, args.warmup, args.reps)
            r['vb_iterations'] = int(fused.ibcc.iterations)
            r['generic_over_fused_of_means'] = r['generic']['mean'] / r['fused']['mean']
            rec.setdefault('end_to_end', {})['e%d' % e] = r
            del fused, generic
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
