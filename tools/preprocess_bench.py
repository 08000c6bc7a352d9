#!/usr/bin/env python3
"""Rate of the on-device input stage (effdet/preprocess.py): 64 seeded 960 x 1280 uint8 frames -> the [64, 3, 640, 640] network
input.  Prints (and with --out writes) the figures DESIGN §8 quotes:

  * `resize_pad_batch` (one launch, bilinear) and `random_resize_pad_batch` drawn with bicubic (one image + one box launch):
    device events over --iters calls after warm-up, median and spread of --rounds windows.  Two figures each: the whole call
    (descriptor packing on the host, the pinned upload, the launches - what a caller waits for) and the image launch alone on
    descriptors packed once (the kernel's own time); achieved bytes / s = (source bytes the pasted windows read + output
    bytes) / time of the launch alone, the bytes computed from the shapes;
  * against the one-image path: the same frames through `resize_pad` in a loop, synchronised at the end, alternated with
    `resize_pad_batch` --rounds times in this process (wall clock around a synchronise for both, so host time counts);
  * against the network: with --ms-per-step (the `ms_per_step` of `python bench.py` from the same visit) the time per 64-image
    batch as a share of the step.

    python tools/preprocess_bench.py --ms-per-step 3.9 --out profiles/preprocess_bench.txt
"""
import argparse
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--height', type=int, default=960)
    ap.add_argument('--width', type=int, default=1280)
    ap.add_argument('--size', type=int, default=640)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--old-iters', type=int, default=10, help='batches per window of the one-image loop (64 calls each)')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--ms-per-step', type=float, default=0.0)
    ap.add_argument('--no-old', action='store_true')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    import torch
    from ood_object_detection_amd.effdet import preprocess as P
    assert torch.cuda.is_available(), 'needs the GPU: a rate measured anywhere else says nothing'
    dev = 'cuda:0'
    B, h, w, S = args.batch, args.height, args.width, args.size
    g = torch.Generator().manual_seed(0)
    frames = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).to(dev) for _ in range(B)]
    fill = P.resolve_fill_color('mean')
    lines = ['# python3 tools/preprocess_bench.py ' + ' '.join(sys.argv[1:])]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def device_windows(fn):
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / args.iters)
        return ms

    def wall(fn, iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / iters

    def traffic(params):
        """bytes the algorithm needs: the source rectangle behind every pasted window once, and the whole output once"""
        src = 0
        for p in params:
            pw, ph = min(S, p.sw - p.ox), min(S, p.sh - p.oy)
            src += 3 * int(pw * w / p.sw) * int(ph * h / p.sh)
        return src + B * 3 * S * S

    out = torch.empty(B, 3, S, S, dtype=torch.uint8, device=dev)

    def launch_alone(params):
        """the image kernel on descriptors packed and uploaded once: no host work inside the timed window but the launch"""
        from ood_object_detection_amd import _lib
        import ctypes
        lib = _lib.load()
        keep, host, devbuf, _, _ = P._pack_params(frames, params)
        fillc = (ctypes.c_int * 3)(*fill)
        st = torch.cuda.current_stream().cuda_stream
        call_args = (st, devbuf.data_ptr(), host.data_ptr(), B, out.data_ptr(), 3 * S * S, S, fillc)
        fn = lambda: _lib.check(lib.effdet_resample_batch_u8(*call_args), 'effdet_resample_batch_u8')
        fn.keep = (keep, host, devbuf, fillc)
        return fn

    say('%d frames %d x %d uint8 -> [%d, 3, %d, %d]' % (B, h, w, B, S, S))
    # eval transform, bilinear
    eval_params = P.resize_pad_params([(h, w)] * B, S)
    ms = device_windows(lambda: P.apply_transforms(frames, eval_params, S, fill, out=out))
    ev = statistics.median(ms)
    nbytes = traffic(eval_params)
    say('resize_pad_batch (bilinear, whole call):      median %.3f ms / batch, spread %.3f .. %.3f  (%d windows of %d)'
        % (ev, min(ms), max(ms), args.rounds, args.iters))
    ms = device_windows(launch_alone(eval_params))
    evk = statistics.median(ms)
    say('  its image launch alone:                     median %.3f ms / batch, spread %.3f .. %.3f; %.1f MB -> %.3f TB/s'
        % (evk, min(ms), max(ms), nbytes / 1e6, nbytes / (evk * 1e-3) / 1e12))
    # train transform, bicubic, with boxes
    random.seed(0)
    train_params = P.draw_train_params([(h, w)] * B, S, (0.4, 1.7), interpolation='bicubic', rng=random)
    boxes = torch.rand(B, 32, 4, generator=g).mul(400).to(dev)
    boxes[..., 2:] += boxes[..., :2]
    cls = torch.randint(1, 90, (B, 32), generator=g).to(dev)
    ms = device_windows(lambda: P.apply_transforms(frames, train_params, S, fill, boxes, cls, out=out))
    tr = statistics.median(ms)
    nbytes = traffic(train_params)
    say('train transform (bicubic, flips, windows, 32 boxes / image, whole call, 2 launches): median %.3f ms / batch, spread %.3f .. %.3f'
        % (tr, min(ms), max(ms)))
    ms = device_windows(launch_alone(train_params))
    trk = statistics.median(ms)
    say('  its image launch alone:                     median %.3f ms / batch, spread %.3f .. %.3f; %.1f MB -> %.3f TB/s'
        % (trk, min(ms), max(ms), nbytes / 1e6, nbytes / (trk * 1e-3) / 1e12))
    if not args.no_old:
        one = torch.stack([P.resize_pad(f, S, fill)[0] for f in frames])
        same = torch.equal(one, P.resize_pad_batch(frames, S, fill).batch)
        say('same bytes as the one-image path: %s' % same)
        assert same
        old, new = [], []
        for _ in range(args.rounds):
            old.append(wall(lambda: [P.resize_pad(f, S, fill) for f in frames], args.old_iters))
            new.append(wall(lambda: P.apply_transforms(frames, eval_params, S, fill, out=out), args.iters))
        say('one-image loop (%d x resize_pad, host clock, synchronised at the end): median %.3f ms / batch, spread %.3f .. %.3f'
            % (B, statistics.median(old), min(old), max(old)))
        say('resize_pad_batch, same clock, alternated:                              median %.3f ms / batch, spread %.3f .. %.3f'
            % (statistics.median(new), min(new), max(new)))
        say('ratio one-image loop / batched: %.1f (slowest batched window against fastest loop window: %.1f)'
            % (statistics.median(old) / statistics.median(new), min(old) / max(new)))
    if args.ms_per_step > 0:
        say('network step (bench.py, same visit) %.3f ms / %d images: eval transform %.1f %% of the step (launch alone %.1f %%), '
            'train transform %.1f %% (launch alone %.1f %%)'
            % (args.ms_per_step, B, 100 * ev / args.ms_per_step, 100 * evk / args.ms_per_step, 100 * tr / args.ms_per_step,
               100 * trk / args.ms_per_step))
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
