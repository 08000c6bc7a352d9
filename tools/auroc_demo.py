"""BASELINE config 4 surrogate: tf_efficientdet_d4 at 1024 px, soft-NMS path, image-level OOD score
max_a(-energy_a) for an "in-distribution" set vs an "OOD" set, AUROC computed on the device.

There is no COCO / OpenImages data (and no trained checkpoint) in this environment, so both sets are synthetic and the
weights are the seeded random initialisation of bench.py: the number demonstrates the pipeline (model -> per-anchor
energy -> image score -> AUROC, all in HIP kernels), not detection quality.  in-dist = smooth low-frequency images,
OOD = white noise.  Prints one JSON line.

    python3 tools/auroc_demo.py [model [size]] [--feature-ood]

--feature-ood adds a detection-level leg and a second JSON line: an `ood_features.FeatureOOD` is fitted on the detections of the
first half of the in-distribution batches, and the detections of the other half and of the OOD set are scored by -energy,
mahalanobis and relative_mahalanobis (all three out of `DetBenchPredict.last_ood`) and compared through `ood.OODEvaluator`.  With
random weights the detections, their classes and therefore every figure of that line mean nothing: it shows that the pieces
connect, no more."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import bench as B
from ood_object_detection_amd import ood
from ood_object_detection_amd.effdet.bench import DetBenchPredict


def main():
    argv = [a for a in sys.argv[1:] if not a.startswith('--')]
    name, size, n_img, bs = (argv[0] if len(argv) > 0 else 'tf_efficientdet_d4'), int(argv[1]) if len(argv) > 1 else 1024, 32, 8
    dev = torch.device('cuda:0')
    model = B.build_model(name, size, 90)
    model.config.soft_nms = True
    model = model.to(dev).to(torch.bfloat16)
    bench = DetBenchPredict(model).to(dev)
    g = torch.Generator(device=dev).manual_seed(7)
    scores = {'in': [], 'ood': []}
    with torch.no_grad():
        for kind in ('in', 'ood'):
            for _ in range(n_img // bs):
                if kind == 'in':
                    low = torch.randn(bs, 3, size // 32, size // 32, device=dev, generator=g)
                    x = torch.nn.functional.interpolate(low, size=(size, size), mode='bilinear', align_corners=False)
                else:
                    x = torch.randn(bs, 3, size, size, device=dev, generator=g)
                bench(x.to(torch.bfloat16))
                scores[kind].append(ood.image_scores(bench.last_ood['anchor_energy']).clone())
    s_in, s_ood = torch.cat(scores['in']), torch.cat(scores['ood'])
    print(json.dumps({'config': '%s %dpx bf16 soft-NMS, %d + %d synthetic images (smooth vs white noise), seeded random weights' % (name, size, n_img, n_img),
                      'score': 'max_a(-energy_a)', 'auroc_in_dist_positive': round(ood.auroc(s_in, s_ood), 4),
                      'mean_score_in': round(float(s_in.mean()), 4), 'mean_score_ood': round(float(s_ood.mean()), 4), 'data': 'synthetic'}))
    if '--feature-ood' in sys.argv[1:]:
        feature_leg(model, name, size, n_img, bs, dev)


def feature_leg(model, name, size, n_img, bs, dev):
    from ood_object_detection_amd.ood_features import FeatureOOD
    g = torch.Generator(device=dev).manual_seed(7)

    def batch(kind):
        if kind == 'in':
            low = torch.randn(bs, 3, size // 32, size // 32, device=dev, generator=g)
            return torch.nn.functional.interpolate(low, size=(size, size), mode='bilinear', align_corners=False).to(torch.bfloat16)
        return torch.randn(bs, 3, size, size, device=dev, generator=g).to(torch.bfloat16)

    plain = DetBenchPredict(model).to(dev)
    feat = FeatureOOD(model.config.fpn_channels, model.config.num_classes, plain.anchors.get_anchors_per_location(), dev)
    n_batches = n_img // bs
    with torch.no_grad():
        for _ in range(n_batches // 2):                                   # fit on the first half of the in-distribution batches
            x = batch('in')
            det = plain(x)
            feat.add_detections(model(x, mode='fpn')[1], det, plain.last_ood['anchor_index'], plain.last_count)
        rows = int(feat.n_c.sum())
        feat.fit(shrinkage=0.01)
        bench = DetBenchPredict(model, feature_ood=feat).to(dev)
        keys = {'-energy': ('energy', True), 'mahalanobis': ('mahalanobis', False), 'relative_mahalanobis': ('relative_mahalanobis', False)}
        cap = n_batches * bs * bench.max_det_per_image
        evs = {k: ood.OODEvaluator(cap, cap, dev) for k in keys}
        for kind, count in (('in', n_batches - n_batches // 2), ('ood', n_batches)):
            for _ in range(count):
                bench(batch(kind))
                for k, (src, neg) in keys.items():
                    evs[k].add_detections(bench.last_ood[src], bench.last_count, kind == 'ood', negate=neg)
    out = {'config': '%s %dpx bf16 soft-NMS, detection level; FeatureOOD fitted on %d detections of %d in-distribution images (shrinkage 0.01)'
                     % (name, size, rows, (n_batches // 2) * bs),
           'note': 'seeded random weights and synthetic images: the detections and their classes are arbitrary, the figures mean nothing',
           'data': 'synthetic'}
    for k, ev in evs.items():
        r = ev.evaluate()
        out[k] = {'auroc': round(r['auroc'], 4), 'aupr_in': round(r['aupr_in'], 4), 'aupr_out': round(r['aupr_out'], 4),
                  'fpr_at_95_tpr': round(r['fpr_at_tpr'], 4), 'n_in': r['n_in'], 'n_ood': r['n_ood']}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
