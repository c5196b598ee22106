#!/usr/bin/env python3
"""bench.py with module attributes of the package set first -- the forms a test seam or a bench record selects, for a
profile of the whole step:

    python tools/bench_with.py trainer._WGRAD_STREAM=False ops.ROUTED_POOL=False -- --mode train --steps 3

Every NAME=VALUE in front of `--` is <module of the package>.<attribute>=<Python literal>; the rest is bench.py's command
line.  The attribute must exist: a typo is an error, not a silent default."""
import ast
import importlib
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    split = sys.argv.index('--')
    for item in sys.argv[1:split]:
        name, value = item.split('=', 1)
        module, attr = name.rsplit('.', 1)
        mod = importlib.import_module('modular_semantic_segmentation_amd.' + module)
        if not hasattr(mod, attr):
            raise SystemExit('%s has no attribute %s' % (mod.__name__, attr))
        setattr(mod, attr, ast.literal_eval(value))
    sys.argv = [os.path.join(ROOT, 'bench.py')] + sys.argv[split + 1:]
    runpy.run_path(sys.argv[0], run_name='__main__')


if __name__ == '__main__':
    main()
