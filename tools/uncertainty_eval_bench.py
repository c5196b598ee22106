#!/usr/bin/env python3
"""Cost of the uncertainty benchmarks' statistic (uncertainty_model.py) at 16 images of 768x384, T = 10 samples, C = 12, three
routes from the same low-resolution sample scores S to the same tables, alternated in one process:
  fused   ops.mc_uncertainty_score: the scoring form of the head, nothing per pixel written;
  maps    ops.mc_uncertainty_head with every map + three ops.uncertainty_stats launches;
  host    the maps to numpy, then uncertainty_model.bin_index + np.add.at (what a user had to do before).
The map-writing head alone is timed beside them (device times by events, mean / min over repetitions; the host route by wall
clock, fewer repetitions), and the statistics kernel's share of the HBM rate from its 16 bytes a pixel (+ 4 with the NLL).
Then a five-temperature BayesianFCN.temperature_search against five independent uncertainty_tables passes (2 images a batch).
Prints one JSON line; --out also writes it.  --kernels-only: a few launches of the two new kernels and the map-writing head
and nothing else (for a kernel trace)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
C, U, H, W, N, T = 12, 64, 384, 768, 16, 10
HBM_BYTES_PER_S = 8e12


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


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--host-reps', type=int, default=2)
    ap.add_argument('--search-reps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--out', default=None, help='also write the JSON record here')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('uncertainty_eval_bench.py needs a GPU')
    from modular_semantic_segmentation_amd import get_model, ops
    from modular_semantic_segmentation_amd import uncertainty_model as um
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    hi, wi = H // 8, W // 8
    g = torch.Generator().manual_seed(0)
    # smooth low-resolution scores with sample-to-sample noise: what dropout samples of one image look like
    base = torch.randn((1, N, hi + 2, wi + 2, C), generator=g) * 2
    S = (base + 0.7 * torch.randn((T, N, hi + 2, wi + 2, C), generator=g)).reshape(T * N, hi + 2, wi + 2, C)
    S[:, 0] = S[:, -1] = 0
    S[:, :, 0] = S[:, :, -1] = 0
    S = S.contiguous().to(dev)
    bias = torch.randn(C, generator=g).to(dev)
    labels = torch.randint(-1, C, (N, H, W), generator=g).to(torch.int32).to(dev)
    npix = N * H * W
    metrics = ops.UNCERTAINTY_METRICS

    def head():
        return ops.mc_uncertainty_head(S, bias, N, hi, wi, C, T, want_mean=True, want_entropy=True, want_cond_entropy=True,
                                       want_variance=True)

    def fused():
        return ops.mc_uncertainty_score(S, bias, N, hi, wi, C, T, labels=labels)

    def bin_maps(out, t):
        for i, key in enumerate(metrics):
            ops.uncertainty_stats(out[key], out['label'], labels, C, mean_prob=out['mean'] if i == 0 else None,
                                  tables={'hist': t['hist'][i], 'nll': t['nll'], 'counts': t['counts']})
        return t

    def maps():
        return bin_maps(head(), ops.uncertainty_tables(C, dev, 3))

    def host():
        out = {k: v.cpu().numpy() for k, v in head().items()}
        lab = labels.cpu().numpy()
        valid = lab >= 0
        wrong = (out['label'][valid] != lab[valid]).astype(np.int64)
        hist = np.zeros((3, 2, 768), np.int64)
        for i, key in enumerate(metrics):
            np.add.at(hist[i], (wrong, um.bin_index(out[key][valid])), 1)
        pl = np.take_along_axis(out['mean'], np.clip(lab, 0, C - 1)[..., None].astype(np.int64), -1)[..., 0][valid]
        nll = np.bincount(lab[valid], weights=-np.log(np.clip(pl.astype(np.float64), 1e-10, 1)), minlength=C)
        return hist, nll

    if args.kernels_only:
        for _ in range(5):
            fused()
            maps()
        torch.cuda.synchronize(dev)
        return
    a, b = fused(), maps()
    assert torch.equal(a['hist'], b['hist']) and torch.equal(a['counts'], b['counts'])
    out = head()
    one = ops.uncertainty_tables(C, dev)
    forms = {'fused': fused, 'maps': maps, 'head_all_maps': head,
             'stats_one_metric': lambda: ops.uncertainty_stats(out['entropy'], out['label'], labels, C, tables=one),
             'stats_with_nll': lambda: ops.uncertainty_stats(out['variance'], out['label'], labels, C, mean_prob=out['mean'],
                                                             tables=one)}
    for _ in range(args.warmup):
        for f in forms.values():
            f()
    times = {k: [] for k in forms}
    for _ in range(args.reps):
        for k, f in forms.items():
            times[k].append(event_time(f, dev))
    rec = {'tool': 'uncertainty_eval_bench', 'shape': [N, H, W], 'num_classes': C, 'num_samples': T, 'reps': args.reps,
           'unit': 's', 'routes': {k: stats(v) for k, v in times.items()}}
    rec['routes']['host'] = stats([wall_time(host, dev) for _ in range(args.host_reps)])
    rec['stats_hbm_fraction'] = {'one_metric_16B_per_pixel': 16.0 * npix / rec['routes']['stats_one_metric']['min'] / HBM_BYTES_PER_S,
                                 'with_nll_20B_per_pixel': 20.0 * npix / rec['routes']['stats_with_nll']['min'] / HBM_BYTES_PER_S}
    rec['fused_over_head'] = rec['routes']['fused']['mean'] / rec['routes']['head_all_maps']['mean']
    # temperature search on the model: one pass of the convolutions per batch against one per temperature
    desc = ({'rgb': 'float32', 'labels': 'int32'}, {'rgb': (None, None, 3), 'labels': (None, None)}, C)
    net = get_model('bayesian_fcn')('rgb', desc, 'rgb', num_units=U, dropout_rate=0.5, num_samples=T, seed=1, batchsize=2,
                                    device=str(dev))
    rng = np.random.default_rng(0)
    data = {'rgb': torch.from_numpy(rng.integers(0, 256, (2, H, W, 3)).astype(np.float32)).to(dev),
            'labels': torch.from_numpy(rng.integers(-1, C, (2, H, W)).astype(np.int32)).to(dev)}
    temps = [0.5, 0.8, 1.0, 1.5, 2.5]
    search = {'temperature_search': lambda: net.temperature_search(data, temps),
              'independent_passes': lambda: [net.uncertainty_tables(data, temperature=t) for t in temps]}
    for f in search.values():
        f()
    st = {k: [] for k in search}
    for _ in range(args.search_reps):
        for k, f in search.items():
            st[k].append(wall_time(f, dev))
    rec['temperature_search'] = {'images': 2, 'temperatures': temps, **{k: stats(v) for k, v in st.items()}}
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
