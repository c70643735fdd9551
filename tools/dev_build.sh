#!/bin/bash
# Fast development build of libgq for kernel A/B experiments: only the flat-scene self-collision Newton variants are instantiated
# (gq_kernels.hip GQ_DEV_ONLY), ~15 s instead of 90.   Usage: tools/dev_build.sh <out .so> [cone 0|1] [extra hipcc flags...]
# The flat self-collision scene is chosen per model (gq_step_call.h model_scene) and a development library carries ONE: add -DGQ_DEV_SELF=1
# for a robot of hulls (mini_cheetah, the headline; hyqreal1, spot), -DGQ_DEV_SELF=2 for one of boxes / capsules / spheres (go2, aliengo,
# hyqreal2) or capsule-proxy mode; without it the library has the kernel with both pair routines (b2, go1), which -DGQ_SCENE_SPLIT_OFF
# gives to every robot.
# It runs `make dev` of gym_quadruped_amd/csrc/Makefile: the product's compiler flags, one translation unit.
# Development builds also read the profiling knobs GQ_STOP_STAGE / GQ_SELF_CUT from the environment (-DGQ_DEV_KNOBS); the product
# library reads no environment variable.
# The result goes under ab/ (git-ignored, travels to the GPU box) and is selected with GQ_LIBGQ_PATH (tools/ab_bench.sh).
set -e
OUT=$(realpath -m "$1"); CONE=${2:-0}; shift; shift || true
make -s -C "$(dirname "$0")/../gym_quadruped_amd/csrc" dev DEV_OUT="$OUT" DEV_CONE="$CONE" DEV_EXTRA="$*"
