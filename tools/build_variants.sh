#!/bin/bash
# Developer aid: build libptrt.so variants with different -D knobs into build/variants/ (travels to the GPU box).
# usage: tools/build_variants.sh name1 "-DPT_STACK_LDS=16" name2 "-DPT_EXT_BLOCK=64" ...
# The objects and each one's compile line are the Makefile's (make -n); every unit is compiled with the knobs, into the variant's own folder.
set -e
cd "$(dirname "$0")/../pathtracing_amd/csrc"
mkdir -p ../../build/variants
objs=$(sed -n 's/^OBJS *:= *//p' Makefile)
while [ $# -ge 2 ]; do
  name=$1; flags=$2; shift 2
  d=../../build/variants/obj_$name; mkdir -p $d
  pids=
  for o in $objs; do make -s -n -B $o | sed "s| -c | $flags -c |; s| -o $o\$| -o $d/$o|" | sh -e & pids="$pids $!"; done
  for p in $pids; do wait $p; done
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../../build/variants/libptrt_$name.so $(for o in $objs; do echo $d/$o; done) -ldl
  echo built $name "($flags)"
done
