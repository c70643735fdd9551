#!/bin/bash
# Register / scratch use of the elliptic production variants of the development build (no library is produced): tools/cone_resources.sh [extra flags]
cd "$(dirname "$0")/../gym_quadruped_amd/csrc"
hipcc $(make -s print-flags) -DGQ_DEV_ONLY=1 "$@" --cuda-device-only -c -o /dev/null -Rpass-analysis=kernel-resource-usage gq_kernels.hip 2>&1 | grep -A9 "Function Name: _ZN2gq11step_kernelILi1ELi0ELb1" | grep "Function Name\|VGPRs:\|ScratchSize" | sed 's/.*remark: *//; s/ \[-Rpass.*//'
