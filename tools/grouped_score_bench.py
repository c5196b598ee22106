#!/usr/bin/env python3
"""Cost of scoring by group at 16 resident images of 768x384, C = 12, with G = 1 and G = 16 (a matrix per image):
  confusion     xv_confusion_matrix_grouped beside xv_confusion_matrix on the same label and prediction maps;
  joint_hist    xv_fused_head_joint_hist_grouped_fwd beside xv_fused_head_joint_hist_fwd on the same low-resolution scores;
  score_groups  BayesFusion.score_groups(data, 'image') -- one pass -- beside 16 calls of score() on one image each: what a
                user had to do for per-image matrices before.
The forms of a comparison alternate in one process; both sides of a kernel comparison are the bare entry points through ctypes.
Device times by events around a window of --launches / --hist-launches launches (kernels: about 0.3 s a window) or 20 calls
(models), after a warm-up of every form; mean / min / std over the windows, per launch or call.  The grouped
results are compared with the ungrouped ones before anything is timed.  Prints one JSON line; --out also writes it
(profiles/grouped_score_bench.json)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
C, U, H, W, N = 12, 64, 384, 768, 16


def event_time(fn, dev, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) * 1e-3 / launches


def stats(v):
    return {'mean': float(np.mean(v)), 'min': float(np.min(v)), 'std': float(np.std(v))}


def alternate(forms, dev, warmup, reps, launches=1):
    for _ in range(warmup):
        for f in forms.values():
            f()
    torch.cuda.synchronize(dev)
    times = {k: [] for k in forms}
    for _ in range(reps):
        for k, f in forms.items():
            times[k].append(event_time(f, dev, launches))
    return {k: stats(v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--launches', type=int, default=20000, help='confusion launches per timed window (about 0.3 s)')
    ap.add_argument('--hist-launches', type=int, default=4000, help='joint-histogram launches per timed window (about 0.3 s)')
    ap.add_argument('--out', default=None, help='also write the JSON record here')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('grouped_score_bench.py needs a GPU')
    from modular_semantic_segmentation_amd import get_model, ops
    from modular_semantic_segmentation_amd.basic_fusion_model import run_lowres_scores
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    rng = np.random.default_rng(0)
    data = {'rgb': torch.from_numpy(rng.integers(0, 256, (N, H, W, 3)).astype(np.float32)).to(dev),
            'depth': torch.from_numpy(rng.integers(0, 65536, (N, H, W, 1)).astype(np.float32)).to(dev),
            'labels': torch.from_numpy(rng.integers(-1, C, (N, H, W)).astype(np.int32)).to(dev)}
    desc = ({'labels': 'int32', 'rgb': 'float32', 'depth': 'float32'},
            {'labels': (None, None), 'rgb': (None, None, 3), 'depth': (None, None, 1)}, C)
    cms = {m: rng.integers(1, 1000, (C, C)) + 20000 * np.eye(C, dtype=np.int64) for m in ('rgb', 'depth')}
    bayes = get_model('bayes_fusion')(confusion_matrices=cms, prefixes={'rgb': 'rgb', 'depth': 'depth'}, data_description=desc,
                                      num_units=U, num_channels={'rgb': 3, 'depth': 1}, expert_model='fcn', batchsize=N,
                                      class_prior='data', seed=1, device=str(dev))
    rec = {'tool': 'grouped_score_bench', 'shape': [N, H, W], 'num_classes': C, 'reps': args.reps,
           'unit': 's per launch / call', 'confusion': {}, 'joint_hist': {}}

    labels = data['labels']
    pred = bayes._predict_batch_impl(data).contiguous()
    Sa, Sb, ba, bb, n, hi, wi = run_lowres_scores(bayes, data)
    groups = {1: np.zeros(N, np.int64), 16: np.arange(N)}
    cm = torch.zeros((C, C), dtype=torch.int64, device=dev)
    hist = torch.zeros((C, C, C), dtype=torch.int64, device=dev)
    ops.confusion_matrix(labels, pred, cm)
    ops.fused_head_joint_hist(Sa, Sb, ba, bb, n, hi, wi, C, labels, hist=hist)
    for G, ids in groups.items():
        # (the group ids are uploaded once: the launches alone are compared)
        dev_ids = torch.from_numpy(ids.astype(np.int32)).to(dev)
        gcm = ops.confusion_matrix_grouped(labels, pred, ids, G, num_classes=C)
        ghist = ops.fused_head_joint_hist_grouped(Sa, Sb, ba, bb, n, hi, wi, C, labels, ids, G)
        assert torch.equal(gcm.sum(0), cm), 'grouped confusion matrices do not sum to the ungrouped one (G = %d)' % G
        assert torch.equal(ghist.sum(0), hist), 'grouped joint histograms do not sum to the ungrouped one (G = %d)' % G
        lib, check, stream = ops._lib.lib(), ops._lib.check, ops._stream()
        # (the timed launches accumulate: into copies, the matrices compared above stay as they are)
        cm_t, hist_t = cm.clone(), hist.clone()
        # both sides of a comparison are the bare entry points through ctypes: the same host cost per launch
        conf_args = (labels.data_ptr(), pred.data_ptr())
        head_args = (Sa.data_ptr(), Sb.data_ptr(), ba.data_ptr(), bb.data_ptr(), n, hi, wi, C, labels.data_ptr())
        forms = {
            'confusion': {
                'grouped': lambda: check(lib.xv_confusion_matrix_grouped(*conf_args, dev_ids.data_ptr(), N, H * W, C, G,
                                                                         gcm.data_ptr(), stream), 'xv_confusion_matrix_grouped'),
                'ungrouped': lambda: check(lib.xv_confusion_matrix(*conf_args, C, N * H * W, cm_t.data_ptr(), stream),
                                           'xv_confusion_matrix')},
            'joint_hist': {
                'grouped': lambda: check(lib.xv_fused_head_joint_hist_grouped_fwd(*head_args, dev_ids.data_ptr(), G,
                                                                                  ghist.data_ptr(), 0, stream),
                                         'xv_fused_head_joint_hist_grouped_fwd'),
                'ungrouped': lambda: check(lib.xv_fused_head_joint_hist_fwd(*head_args, hist_t.data_ptr(), 0, stream),
                                           'xv_fused_head_joint_hist_fwd')}}
        for name, launches in (('confusion', args.launches), ('joint_hist', args.hist_launches)):
            r = alternate(forms[name], dev, args.warmup, args.reps, launches)
            r['grouped_over_ungrouped'] = r['grouped']['mean'] / r['ungrouped']['mean']
            r['launches_per_window'] = launches
            rec[name][str(G)] = r

    # the model: one grouped pass against a score() per image
    singles = [{k: v[i:i + 1] for k, v in data.items()} for i in range(N)]
    per_image = bayes.score_groups(data, 'image')
    assert all(np.array_equal(per_image[i][1], bayes.score(singles[i])[1]) for i in (0, N - 1))
    r = alternate({'score_groups_image': lambda: bayes.score_groups(data, 'image'),
                   'score_per_image': lambda: [bayes.score(s) for s in singles],
                   'score_once': lambda: bayes.score(data)}, dev, args.warmup, args.reps, 20)
    r['calls_per_window'] = 20
    r['speedup_of_means'] = r['score_per_image']['mean'] / r['score_groups_image']['mean']
    rec['score_groups'] = r
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
