#!/usr/bin/env python3
"""conv_dtype='fp32' (the label-exact parity mode) timed like the headline: two SimpleFCN experts + Bayes fusion on
resident 768x384 RGB-D inputs.  Prints one JSON record.  usage: exact_bench.py [batch] [steps] [--scalar]
(--scalar: round 4's vector-ALU conv kernel, fcn_exact.SCALAR_KERNEL -- the A/B baseline)"""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def main():
    from modular_semantic_segmentation_amd import fcn_exact
    fcn_exact.SCALAR_KERNEL = '--scalar' in sys.argv
    argv = [a for a in sys.argv if a != '--scalar']
    batch = int(argv[1]) if len(argv) > 1 else 16
    steps = int(argv[2]) if len(argv) > 2 else 3
    dev = torch.device('cuda', 0)
    net = bench.build_model(dev, 'bayes', 'fcn', batch, 'fp32')
    data = bench.synthetic_batch(dev, batch, 384, 768, seed=5)
    if os.environ.get('XV_ZERO', '0') == '1':       # diagnostic: no operand toggles (is the steady state clock-bound?)
        import numpy as np
        for key in list(net.variables):
            if 'upscore' not in key and key.rsplit('/', 1)[-1] in ('kernel', 'bias'):
                net.variables[key] = np.zeros_like(net.variables[key])
        net._variables_changed()
        data = {k: torch.zeros_like(v) for k, v in data.items()}
    net._predict_batch(data)
    torch.cuda.synchronize()
    tr = time.perf_counter()
    while time.perf_counter() - tr < 1.5:       # clock ramp out of idle (as bench.py)
        net._predict_batch(data)
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        net._predict_batch(data)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    fl = batch * (bench.conv_flops_per_image(384, 768, 3) + bench.conv_flops_per_image(384, 768, 1))
    from modular_semantic_segmentation_amd import ops
    prof = []
    net.concurrent_experts = False
    net._predict_batch(data)
    ops.CONV_PROFILE = prof
    net._predict_batch(data)
    torch.cuda.synchronize()
    ops.CONV_PROFILE = None
    for kind, f, e0, e1 in prof:
        ms = e0.elapsed_time(e1)
        print('  %-6s %8.2f GF %9.1f us %7.1f TF/s' % (kind, f / 1e9, ms * 1e3, f / ms / 1e9), file=sys.stderr)
    k3 = [(f, e0.elapsed_time(e1)) for kind, f, e0, e1 in prof if kind == 'k3f32']
    print(json.dumps({'workload': 'two SimpleFCN experts + Bayes fusion 768x384, conv_dtype=fp32', 'batch': batch,
                      'ms_per_step': round(dt * 1e3, 3), 'images_per_s': round(batch / dt, 2),
                      'conv_tflops': round(fl / dt / 1e12, 2),
                      'conv3x3_tflops_serial': round(sum(f for f, _ in k3) / sum(m for _, m in k3) / 1e9, 2),
                      'scalar_kernel': fcn_exact.SCALAR_KERNEL}))


if __name__ == '__main__':
    main()
