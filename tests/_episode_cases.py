"""What the GPU tests of the episode stage share (test_episode_gpu.py, test_episode_loss_gpu.py, test_support_loss_gpu.py): the
MetaHead-like inputs of the chain, the bit comparison of two runs and the seeded d0 MetaHead + ProjectionNet of the end-to-end tests."""
import torch

import _episode_ref as ref

DEV = 'cuda:0'
A = 9
OFFSET = 2                          # supp_level_offset
SIDES = [32, 16, 8, 4, 2]           # 256 px
NUM_IMAGES = 25


def _head_like(vals, side):
    """vals [B, N] -> [B, A, H, W] view of [B, H, W, A] memory inside a larger per-image buffer, as the MetaHead returns it"""
    B, N = vals.shape
    buf = torch.zeros(B, N + 45, device=DEV)
    buf[:, :N] = vals.to(DEV)
    return buf[:, :N].view(B, side, side, A).permute(0, 3, 1, 2)


def _levels(seed, B, Fc, sides):
    gen = torch.Generator().manual_seed(seed)
    activs = [torch.randn(B, s, s, Fc, generator=gen).to(DEV).permute(0, 3, 1, 2) for s in sides]
    confs = [_head_like(ref.tie_free_confs(seed + s, B, A * s * s), s) for s in sides]
    return activs, confs


def _same(a, b):
    return all(torch.equal(x, y) or bool((torch.isnan(x) == torch.isnan(y)).all() and torch.equal(x.nan_to_num(), y.nan_to_num()))
               for x, y in zip(a, b))


def _device_sel(sel):
    return {k: v.to(DEV) for k, v in sel.items()}


def _meta_head(golden, seed, with_case=False):
    """-> the seeded MetaHead, a 106 -> 512 -> 256 ProjectionNet and the level inputs; with_case: the meta_nets case in front"""
    from _seeded import meta_nets_case
    from ood_object_detection_amd.effdet.config import get_efficientdet_config
    from ood_object_detection_amd.effdet.efficientdet import MetaHead, ProjectionNet
    c = meta_nets_case(golden('meta_nets'))
    cfg = get_efficientdet_config('tf_efficientdet_d0')
    torch.manual_seed(seed)
    mh = MetaHead(cfg, pretrain_init=c['init'])
    with torch.no_grad():
        mh.predict_pw.copy_(c['extra']['predict_pw']); mh.predict_pb.copy_(c['extra']['predict_pb'])
    proj_net = ProjectionNet(cfg, 512)                                          # 106 -> 512 -> 256
    with torch.no_grad():
        proj_net.dot_mult.fill_(1.5); proj_net.dot_add.fill_(0.25)
    gen = torch.Generator().manual_seed(seed)
    xs = [torch.randn(NUM_IMAGES, c['F'], s, s, generator=gen) for s in SIDES]
    out = (mh.to(DEV), proj_net.to(DEV), xs)
    return (c,) + out if with_case else out
