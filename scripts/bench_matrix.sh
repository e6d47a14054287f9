#!/bin/bash
# bench.py --full (kernel rooflines; no CPU baseline) over the BASELINE.json
# configs that fit one GPU, run from the repo root on an MI355X:
#   bash scripts/bench_matrix.sh [TAG] [OUTDIR]   -> OUTDIR/bm_TAG_<config>.json / .err
set -o pipefail
TAG=${1:-m}
OUT=${2:-bench_out}
mkdir -p $OUT
B="python bench.py --full --no-cpu-baseline"
timeout -k 10 400 $B --steps 5 --warmup 2 > $OUT/bm_${TAG}_base.json 2> $OUT/bm_${TAG}_base.err && \
timeout -k 10 300 $B --model tiny --steps 5 --warmup 2 > $OUT/bm_${TAG}_tiny.json 2> $OUT/bm_${TAG}_tiny.err && \
timeout -k 10 300 $B --model small --steps 5 --warmup 2 > $OUT/bm_${TAG}_small.json 2> $OUT/bm_${TAG}_small.err && \
timeout -k 10 300 $B --model small-q5_1 --steps 5 --warmup 2 > $OUT/bm_${TAG}_smallq5.json 2> $OUT/bm_${TAG}_smallq5.err && \
timeout -k 10 300 $B --clips-per-gpu 8 --steps 3 --warmup 1 > $OUT/bm_${TAG}_base8.json 2> $OUT/bm_${TAG}_base8.err && \
timeout -k 10 500 $B --model large-v3 --beam 5 --steps 2 --warmup 1 > $OUT/bm_${TAG}_lv3b5.json 2> $OUT/bm_${TAG}_lv3b5.err && \
timeout -k 10 400 $B --model large-v3 --steps 2 --warmup 1 > $OUT/bm_${TAG}_lv3.json 2> $OUT/bm_${TAG}_lv3.err
echo "EXIT $?"
