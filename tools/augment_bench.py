#!/usr/bin/env python3
"""Cost of training augmentation on the device against the host chain, at what SYNTHIA training runs: batches of 16 images
from a synthetic pool of 1280x760 sources under the shipped TRAIN_AUGMENTATION (240 x 240 crops), and under the same with the
shear probability raised to 1 (every stage can nest: the kernel's worst case).  Per configuration:
  launch_us       xv_augment_batch alone on a fixed drawn batch (device events around one launch, warmed up)
  batch_us        draw + pack + upload + launch, as DeviceTrainset.training_batches does it (host clock, synchronised)
  host_ms         `augmentate` + crop_multiple + float cast per sample on one core (host clock)
  train_step_us   the 16-image FCN training step of this run on the 240 x 240 batch, and both device figures over it
Four images of each timed batch are compared with the host chain (equal, or the tool fails).  No target: the record is the result.
Prints one JSON line; --out also writes it (profiles/augment_bench.json)."""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H, W, N, POOL = 760, 1280, 16, 16


def stats(v):
    return {'mean': float(np.mean(v)), 'min': float(np.min(v)), 'std': float(np.std(v))}


def make_pool(seed=0):
    """smooth synthetic images: blocks of 8 x 8 equal pixels plus noise (bilinear taps then differ, like a photograph)"""
    rng = np.random.default_rng(seed)
    up = lambda a: np.repeat(np.repeat(a, 8, axis=1), 8, axis=2)
    rgb = np.clip(up(rng.integers(0, 256, (POOL, H // 8, W // 8, 3))) + rng.integers(-8, 9, (POOL, H, W, 3)), 0, 255)
    depth = np.clip(up(rng.integers(0, 65536, (POOL, H // 8, W // 8))) + rng.integers(-300, 301, (POOL, H, W)), 0, 65535)
    return {'rgb': rgb.astype(np.uint8), 'depth': depth.astype(np.uint16),
            'labels': up(rng.integers(0, 12, (POOL, H // 8, W // 8))).astype(np.int32)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--host-samples', type=int, default=4)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'augment_bench needs a GPU'
    dev = torch.device('cuda:0')
    from modular_semantic_segmentation_amd import get_model, ops
    from modular_semantic_segmentation_amd.datasets import augmentation as aug
    from modular_semantic_segmentation_amd.datasets.device_augmentation import DeviceTrainset
    from modular_semantic_segmentation_amd.datasets.synthia_cityscapes import TRAIN_AUGMENTATION

    host_pool = make_pool()
    configs = {'shipped': dict(TRAIN_AUGMENTATION),
               'shear_always': dict(TRAIN_AUGMENTATION, shear=[1] + list(TRAIN_AUGMENTATION['shear'][1:]))}
    rec = {'source': [H, W], 'batch': N, 'pool': POOL, 'reps': args.reps}
    first_batch = None
    for name, config in configs.items():
        trainset = DeviceTrainset(host_pool, config, dev)
        random.seed(1)
        np.random.seed(1)
        items = np.arange(N, dtype=np.int32)
        plans, records, tables = trainset.draw_batch(items)
        out = ops.augment_batch(trainset.pool, items, records, tables)
        # equal to the host chain (the first four images: the host takes seconds per sample), or these are times of
        # something else
        for n in range(4):
            blob = aug.apply_augmentation({m: v[n].copy() for m, v in host_pool.items()}, plans[n])
            for m, t in zip(('rgb', 'depth', 'labels'), out):
                assert np.array_equal(t[n].cpu().numpy().reshape(blob[m].shape), blob[m]), (name, n, m)
        if first_batch is None:
            first_batch = {'rgb': out[0].clone(), 'labels': out[2].clone()}
        stage_counts = {k: sum(p[k] is not None for p in plans) for k in ('scale', 'rotate', 'shear')}

        # the launch alone (with its small upload, which ops.augment_batch makes part of the call): device events
        launch = []
        for i in range(args.warmup + args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ops.augment_batch(trainset.pool, items, records, tables)
            b.record()
            torch.cuda.synchronize(dev)
            if i >= args.warmup:
                launch.append(a.elapsed_time(b) * 1e3)
        # draw + pack + upload + launch: the iterator, host clock around a synchronised batch
        batches = trainset.training_batches(N)
        whole = []
        for i in range(args.warmup + args.reps):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            next(batches)
            torch.cuda.synchronize(dev)
            if i >= args.warmup:
                whole.append((time.perf_counter() - t0) * 1e6)
        # the host chain, one core
        host = []
        for n in range(args.host_samples):
            blob = {m: v[n].copy() for m, v in host_pool.items()}
            t0 = time.perf_counter()
            blob = aug.augmentate(blob, **config)
            blob = {m: np.asarray(aug.crop_multiple(v)).astype('int32' if m == 'labels' else 'float32') for m, v in blob.items()}
            host.append((time.perf_counter() - t0) * 1e3)
        rec[name] = {'stages_in_timed_batch': stage_counts, 'launch_us': stats(launch), 'batch_us': stats(whole),
                     'host_ms_per_sample': stats(host)}

    # the 16-image training step of this run, on a batch the device made
    desc = ({'rgb': 'float32', 'labels': 'int32'}, {'rgb': (None, None, 3), 'labels': (None, None)}, 12)
    net = get_model('fcn')('rgb', desc, 'rgb', num_units=64, batch_normalization=False, batchsize=N, learning_rate=1e-4,
                           trainer='adam', sync_loss=False)
    step = []
    for i in range(args.warmup + 20):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        net._train_batch(first_batch)
        b.record()
        torch.cuda.synchronize(dev)
        if i >= args.warmup:
            step.append(a.elapsed_time(b) * 1e3)
    rec['train_step_us'] = stats(step)
    for name in configs:
        rec[name]['launch_over_step'] = rec[name]['launch_us']['mean'] / rec['train_step_us']['mean']
        rec[name]['batch_over_step'] = rec[name]['batch_us']['mean'] / rec['train_step_us']['mean']
        rec[name]['host_batch_over_step'] = rec[name]['host_ms_per_sample']['mean'] * 1e3 * N / rec['train_step_us']['mean']
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
