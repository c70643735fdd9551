#!/bin/bash
# Annotated ISA of the development build's headline kernel + its resource line: tools/isa_dev.sh <tag> [extra flags]  ->  /tmp/isa/<tag>.txt
TAG=$1; shift
mkdir -p /tmp/isa
cd "$(dirname "$0")/../gym_quadruped_amd/csrc"
hipcc $(make -s print-flags) -DGQ_DEV_ONLY=0 -DGQ_DEV_SELF=1 -gline-tables-only -S --cuda-device-only "$@" -o /tmp/isa/$TAG.s gq_kernels.hip 2>&1 | grep -v "warning\|^$" | head
cd ../..
K=step_kernelILi1ELi0ELb0ELb0ELb1ELb0ELb0E   # mini_cheetah on flat: SCENE_FLAT_SELF_HULL (-DGQ_DEV_SELF=1)
python tools/isa_walk.py /tmp/isa/$TAG.s $K /tmp/isa/$TAG.txt
echo "instructions $(grep -vc ':$' /tmp/isa/$TAG.txt)  s_waitcnt $(grep -c s_waitcnt /tmp/isa/$TAG.txt)  s_load $(grep -c s_load_dword /tmp/isa/$TAG.txt)  scratch $(grep -c scratch_ /tmp/isa/$TAG.txt)"
awk "/^_ZN2gq11$K/{f=1} f&&/; (NumVgprs|NumSgprs|ScratchSize|Occupancy)/{printf \"%s \", \$0} f&&/Occupancy/{print \"\"; exit}" /tmp/isa/$TAG.s
