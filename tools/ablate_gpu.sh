#!/bin/bash
# Phase ablation of the fused MBConv kernels (skip expand / depthwise / both): uses the separate -DEFFDET_ABLATE build
# (libeffdet_hip_ablate.so, `make -C ood_object_detection_amd/csrc ablate`); the product library has no such switch.
REPO=${GRAFT_REPO_ROOT:-/root/repo}
cd $REPO
OUT=${BENCH_OUT:-bench_out}; mkdir -p $OUT
make -C ood_object_detection_amd/csrc ablate > $OUT/abl_build.log 2>&1 || exit 1
for d in 0 1 2 3; do
  EFFDET_DEBUG_SKIP=$d timeout -k 10 300 python tools/ablate_run.py --full --steps 5 --warmup 2 --no-cpu-baseline --profile-out $OUT/abl_$d.txt > $OUT/abl_$d.log 2>&1
done
