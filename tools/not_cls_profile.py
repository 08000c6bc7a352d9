#!/usr/bin/env python
"""One differentiable `mode='not_cls'` forward + backward (BiFPN + box head, pyramid handed out) at infer.py's default model:
tf_efficientdet_d3 (F = 160, six cells, four box repeats), 640 px, float32, the query batch of the default flags
(n_way 1 x num_qry 25 images), BatchNorm frozen as freeze_fpn_bn / freeze_box_bn leave it.  The backbone features are random
tensors of the right shapes (the stage does not care), every pyramid level and the boxes get a gradient.

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python3 tools/not_cls_profile.py
    ROCPROF_AFTER_GAP_MS=300 python3 tools/summarize_rocprof.py <dir> <out>      the last iteration alone (table mode)
    python3 tools/not_cls_profile.py --time 20                                   HIP-event time per iteration
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from ood_object_detection_amd.effdet.config import get_efficientdet_config  # noqa: E402
from ood_object_detection_amd.effdet.efficientdet import EfficientDet  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--model', default='tf_efficientdet_d3')
    ap.add_argument('--size', type=int, default=640)
    ap.add_argument('--batch', type=int, default=25)
    ap.add_argument('--time', type=int, default=0, help='timed iterations after the warm-up (0: one iteration behind an idle gap)')
    a = ap.parse_args()
    torch.manual_seed(0)
    cfg = get_efficientdet_config(a.model)
    cfg.image_size = (a.size, a.size)
    cfg.num_classes = 1
    cfg.backbone_args = dict(drop_path_rate=0.0)
    model = EfficientDet(cfg, pretrained_backbone=False).cuda().float().train()
    model.apply(lambda m: m.eval() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm) else None)
    feats = [torch.randn(a.batch, i['num_chs'], a.size // i['reduction'], a.size // i['reduction'], device='cuda').requires_grad_()
             for i in model.fpn.in_feature_info]
    g = None

    def step():
        nonlocal g
        model.zero_grad(set_to_none=True)
        for f in feats:
            f.grad = None
        activs, box = model(feats, mode='not_cls')
        outs = list(activs) + list(box)
        if g is None:
            g = [torch.randn_like(o) for o in outs]
        torch.autograd.backward(outs, g)

    for _ in range(3):                      # the first two record and upload the stage tables
        step()
    torch.cuda.synchronize()
    if a.time <= 0:
        time.sleep(0.5)                     # an idle gap in the trace: what follows is one table-mode iteration
        step()
        torch.cuda.synchronize()
        print('one not_cls forward + backward: %s, %d px, %d images' % (a.model, a.size, a.batch))
        return
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(a.time):
        step()
    t1.record()
    torch.cuda.synchronize()
    print('not_cls forward + backward, %s %d px %d images float32: %.2f ms per iteration (mean of %d, HIP events, host launch '
          'overhead included), peak memory %.1f GiB' % (a.model, a.size, a.batch, t0.elapsed_time(t1) / a.time, a.time,
                                                         torch.cuda.max_memory_allocated() / 2.0 ** 30))


if __name__ == '__main__':
    main()
