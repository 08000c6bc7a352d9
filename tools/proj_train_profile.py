#!/usr/bin/env python
"""ProjectionNet training forward + backward (input and weight gradients) at infer.py's d3 defaults: 25 images x
(72 + 144 + 36) anchors on P5-P7 = 6 300 rows, K = fpn_channels 160 + 42 = 202, width 512 -> 256, proj_depth 2.

    rocprofv3 --kernel-trace --stats ... -- python3 tools/proj_train_profile.py             one iteration: the launch record
    python3 tools/proj_train_profile.py --time 50                                            HIP-event time per iteration
"""
import argparse
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from ood_object_detection_amd.effdet.aux_nets import ProjectionNet  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=6300)
    ap.add_argument('--fpn', type=int, default=160)
    ap.add_argument('--width', type=int, default=512)
    ap.add_argument('--depth', type=int, default=2)
    ap.add_argument('--time', type=int, default=0, help='timed iterations after 5 warm-up ones (0: one untimed iteration)')
    a = ap.parse_args()
    torch.manual_seed(0)
    net = ProjectionNet(types.SimpleNamespace(fpn_channels=a.fpn), a.width, proj_depth=a.depth).cuda()
    x = torch.randn(a.rows, a.fpn + 42).cuda().requires_grad_(True)
    gy = torch.randn(a.rows, a.width // 2).cuda()
    torch.cuda.synchronize()

    def step():
        net.zero_grad(set_to_none=True)
        x.grad = None
        net(x).backward(gy)

    if a.time <= 0:
        step()
        torch.cuda.synchronize()
        print('one forward + backward: rows %d, K %d, %d -> %d, depth %d' % (a.rows, a.fpn + 42, a.width, a.width // 2, a.depth))
        return
    for _ in range(5):
        step()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(a.time):
        step()
    t1.record()
    torch.cuda.synchronize()
    print('forward + backward: %.1f us per iteration (mean of %d, HIP events, host launch overhead included)'
          % (t0.elapsed_time(t1) * 1e3 / a.time, a.time))


if __name__ == '__main__':
    main()
