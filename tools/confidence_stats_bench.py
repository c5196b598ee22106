#!/usr/bin/env python3
"""Cost of the uncertainty benchmarks' tables of a fused posterior (csrc/confidence_stats.hip) at 16 images of 768x384, C = 12,
for two, three and four experts and the three fusion modes; three routes from the same low-resolution scores to the same
tables, alternated in one process:
  fused   ops.fused_head_multi_confidence_stats: one launch, nothing per pixel written;
  maps    ops.fused_head_multi_confidence with all four maps + three ops.uncertainty_stats launches on 1 - map values made by
          torch (what the device offered before);
  host    the maps to numpy, then uncertainty_model.confidence_tables_reference (what predict_confidence users had to do).
Device times by events (mean / min over repetitions), the host route by wall clock with fewer repetitions.  The fused launch
with every expert's own tables beside the fusion's is timed too.  Prints one JSON line; --out also writes it."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
C, H, W, N = 12, 384, 768, 16
MODES = ('bayes', 'dirichlet', 'mean')


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


def fusion_tables(mode, E, g, dev):
    if mode == 'mean':
        return {}
    cond = torch.rand((E, C, C), generator=g) + 0.05 + 2.0 * torch.eye(C)
    logprior = torch.log_softmax(torch.randn(C, generator=g), 0).contiguous().to(dev)
    if mode == 'bayes':
        return dict(tab=torch.log(cond / cond.sum(1, keepdim=True)).contiguous().to(dev), logprior=logprior)
    am1 = (torch.rand((E, C, C), generator=g) * 0.3 + 0.5 * torch.eye(C)).contiguous()
    return dict(tab=am1.to(dev), lognorm=torch.randn((E, C), generator=g).contiguous().to(dev), logprior=logprior)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--host-reps', type=int, default=1)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None, help='also write the JSON record here')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('confidence_stats_bench.py needs a GPU')
    from modular_semantic_segmentation_amd import ops
    from modular_semantic_segmentation_amd import uncertainty_model as um
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    hi, wi = H // 8, W // 8
    g = torch.Generator().manual_seed(0)
    # smooth low-resolution scores, every expert the shared field plus its own noise: what experts on one scene look like
    shared = torch.randn((N, hi, wi, C), generator=g) * 3.0
    S, bias = [], []
    for _ in range(4):
        s = torch.zeros((N, hi + 2, wi + 2, C))
        s[:, 1:-1, 1:-1] = shared + 1.5 * torch.randn((N, hi, wi, C), generator=g)
        S.append(s.contiguous().to(dev))
        bias.append(torch.randn(C, generator=g).to(dev))
    labels = torch.randint(-1, C, (N, H, W), generator=g).to(torch.int32).to(dev)
    labels_h = labels.cpu().numpy()
    rec = {'tool': 'confidence_stats_bench', 'shape': [N, H, W], 'num_classes': C, 'reps': args.reps, 'unit': 's', 'cases': {}}
    for E in (2, 3, 4):
        for mode in MODES:
            t = fusion_tables(mode, E, g, dev)
            head = (S[:E], bias[:E], N, hi, wi, C, mode)

            def fused():
                return ops.fused_head_multi_confidence_stats(*head, labels, 1.0, **t)

            def fused_experts():
                return ops.fused_head_multi_confidence_stats(*head, labels, 1.0, experts=True, **t)

            def write_maps():
                return ops.fused_head_multi_confidence(*head, 1.0, want=('label', 'confidence', 'entropy', 'margin'), **t)

            def maps():
                out = write_maps()
                tables = ops.uncertainty_tables(C, dev, 3)
                for i, v in enumerate((out['entropy'], 1.0 - out['confidence'], 1.0 - out['margin'])):
                    ops.uncertainty_stats(v, out['label'], labels, C,
                                          tables={'hist': tables['hist'][i], 'nll': tables['nll'], 'counts': tables['counts']})
                return tables

            def host():
                out = {k: v.cpu().numpy() for k, v in write_maps().items()}
                return um.confidence_tables_reference(out, out['label'], labels_h, num_classes=C)

            a, b = fused(), maps()
            assert torch.equal(a['hist'], b['hist'])
            forms = {'fused': fused, 'fused_with_expert_tables': fused_experts, 'maps': maps, 'head_all_maps': write_maps}
            for _ in range(args.warmup):
                for f in forms.values():
                    f()
            times = {k: [] for k in forms}
            for _ in range(args.reps):
                for k, f in forms.items():
                    times[k].append(event_time(f, dev))
            case = {k: stats(v) for k, v in times.items()}
            if mode == 'bayes':                              # (the host route does not depend on the mode: once per expert count)
                case['host'] = stats([wall_time(host, dev) for _ in range(args.host_reps)])
            case['fused_over_maps'] = case['fused']['mean'] / case['maps']['mean']
            rec['cases']['E%d_%s' % (E, mode)] = case
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
