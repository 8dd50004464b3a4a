#!/bin/bash
# A/B timing of library variants (dev tool): every ab/*.so is copied over the in-tree library and benched.
set -e
LIB=nerf_for_angiography_amd/csrc/libafx.so
cp $LIB /tmp/libafx_orig.so
for v in ab/*.so; do
  cp $v $LIB
  n=$(basename $v .so)
  python bench.py --full --no-cpu "$@" > ab/$n.log 2>&1 || { echo "$v FAILED"; tail -3 ab/$n.log; continue; }
  grep "^\[stamps\]" ab/$n.log | head -8 || true
  grep "^{" ab/$n.log | tail -1 | python -c "import json,sys; d=json.loads(sys.stdin.read()); print('$v', d['ms_per_step'], d['roofline']['kernel_ms_per_step'], d.get('final_loss'))"
done
cp /tmp/libafx_orig.so $LIB
