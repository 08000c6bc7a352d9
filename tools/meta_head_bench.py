#!/usr/bin/env python
"""Time of MetaHead's no-grad forward (effdet/meta_head.py: one effdet_sepconv_meta + one effdet_bn_batch_stats launch per layer,
then the predict launch) at episode sizes: 25 images of 256 px, the five pyramid levels 32 .. 2 (the query pass) and P5 - P7
alone (`level_offset=2`, the support pass), d0 and d5 widths, float32 and bf16.

    python3 tools/meta_head_bench.py                       the library of this tree
    python3 tools/meta_head_bench.py --lib other/libeffdet_hip.so
                                                           another build of the same ABI, for a before / after pair (a build
                                                           whose statistics table had 2 rows per tile runs in the 3-row table)

`--rounds` windows of `--iters` forwards each (HIP events around a window, host launch overhead included - the head is launch
bound at these sizes); the report is the median window and the min .. max spread.  Run the two builds alternately in one
session and compare the difference with that spread.  Needs the GPU: there is no fallback."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import torch  # noqa: E402

import _meta_head_cases as mc  # noqa: E402
from ood_object_detection_amd import _lib  # noqa: E402


def window(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lib', default=None, help='time this build of libeffdet_hip.so instead of the tree\'s')
    ap.add_argument('--images', type=int, default=25)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=7)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'meta_head_bench.py needs an MI355X'
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    _lib.load()
    dev = 'cuda:0'
    sizes = [32, 16, 8, 4, 2]
    print('library %s' % _lib.LIB_PATH)
    for name in ('tf_efficientdet_d0', 'tf_efficientdet_d5'):
        for dtype in (torch.float32, torch.bfloat16):
            cfg, _, _, mh = mc.build_meta_head(name, 1)
            mh = mh.to(dev).to(dtype)
            x = [t.to(dev).to(dtype) for t in mc.level_inputs(1, cfg.fpn_channels, [(s, s) for s in sizes], batch=a.images)]
            for off in (0, 2):
                with torch.no_grad():
                    fn = lambda: mh(x, level_offset=off)
                    for _ in range(10):
                        fn()
                    torch.cuda.synchronize()
                    w = [window(fn, a.iters) for _ in range(a.rounds)]
                print('F %3d %-8s levels %d..4: median %7.1f us (min %7.1f, max %7.1f) per forward, %d images'
                      % (cfg.fpn_channels, str(dtype).split('.')[1], off, statistics.median(w), min(w), max(w), a.images))


if __name__ == '__main__':
    main()
