#!/usr/bin/env python3
"""Record tests/golden/chooser_geometry.json from the built library: what xv_conv2d_choose_cfg answers and how many bytes
the three filter-gradient workspace queries ask for, over the conv layers of the BASELINE.json input sizes.

TEST INFRASTRUCTURE.  The queries are host arithmetic and launch nothing; the only device fact they read is the CU count
(256 where there is no device, and on MI355X), which the file records.  Run it on the commit whose answers are to be
pinned -- tests/test_host_logic.py::test_chooser_and_workspace_geometry_pinned compares a later build against the file.

Usage:  python tests/golden/make_chooser_golden.py     (from the repo root, after build())
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from modular_semantic_segmentation_amd import _lib  # noqa: E402
from modular_semantic_segmentation_amd.fcn import ENCODER  # noqa: E402

SIZES = ((256, 512), (384, 768), (512, 1024), (1024, 2048))     # (h, w) of the BASELINE.json configurations
BATCHES = (1, 8, 16)             # 384x768 at 1 and 16 images: the 48x96 conv4 and 24x48 conv5 maps the chooser has rules for
UNITS = (64, 128)                # padded widths of the 1x1 score convs


def conv_layers(h, w):
    """(h, w, cin, cout) of every MFMA conv of one FCN expert on an h x w input: conv1_2 .. conv5_3, the two score convs"""
    out, cin = [], None
    for name, cout, pool in ENCODER:
        if cin is not None:
            out.append((h, w, cin, cout))
        cin = cout
        if pool is not None:
            h, w = h // 2, w // 2
    # (ENCODER ends at conv5_3 on the pool4 map; score_conv4 reads conv4_3, one level up)
    for up in UNITS:
        out += [(2 * h, 2 * w, 512, up), (h, w, 512, up)]
    return sorted(set(out))


def record(lib):
    bf16, fp8 = _lib.CONSTANTS['XV_BF16'], _lib.CONSTANTS['XV_FP8']
    pairs = ((bf16, bf16), (bf16, fp8), (fp8, bf16), (fp8, fp8))
    choose, wgrad, first, score = {}, {}, {}, {}
    for h0, w0 in SIZES:
        for n in BATCHES:
            for h, w, cin, cout in conv_layers(h0, w0):
                for k in (1, 3):
                    key = '%d,%d,%d,%d,%d,%d' % (n, h, w, cin, cout, k)
                    # 32 answers per layer: dtype pair major, flags 0..7 minor (negative = the XV_E* code for that combination)
                    choose[key] = [lib.xv_conv2d_choose_cfg(n, h, w, cin, cout, k, i, o, f) for i, o in pairs for f in range(8)]
                    wgrad[key] = lib.xv_conv2d_bwd_filter_workspace_bytes(n, h, w, cin, cout, k)
            for cin in (1, 3):
                first['%d,%d,%d,%d' % (n, h0, w0, cin)] = lib.xv_conv2d_first_bwd_filter_workspace_bytes(n, h0, w0, cin)
            score['%d,%d,%d' % (n, h0, w0)] = lib.xv_score_dense_bwd_workspace_bytes(n, h0, w0)
    return {'num_cus': lib.xv_conv2d_stats_rows(),
            'dtype_pairs': [[i, o] for i, o in pairs],
            'choose_cfg': choose,
            'bwd_filter_workspace_bytes': wgrad,
            'first_bwd_filter_workspace_bytes': first,
            'score_dense_bwd_workspace_bytes': score}


if __name__ == '__main__':
    table = record(_lib.lib())
    with open(os.path.join(HERE, 'chooser_geometry.json'), 'w') as f:
        json.dump(table, f, separators=(',', ':'), sort_keys=True)
        f.write('\n')
    print('recorded %d layers at %d CUs' % (len(table['choose_cfg']), table['num_cus']))
