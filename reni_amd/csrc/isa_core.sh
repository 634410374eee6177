#!/bin/bash
# Emit the gfx950 ISA of one translation unit, with build.sh's flags.
# Usage: isa_core.sh UNIT OUT.s [extra hipcc flags]
#   UNIT is one of build.sh's list: core main_f32 main_bf16 film_f32 film_bf16 train_film wide shade image raster raster_bwd silhouette
#   camera meshreg points pointmesh knn baselines diffuse glossy glossy_bwd resample rotate metrics lights visibility texture splitsum
# Two builds compare with
#   sed -E 's/__hip_cuid_[0-9a-f]+/__hip_cuid_X/g' OUT.s | sha256sum
# (the cuid symbol is a hash of the source text, everything else is the code object).
set -e
out="$(realpath -m "${2:-}")"
cd "$(dirname "$0")"
units="core main_f32 main_bf16 film_f32 film_bf16 train_film wide shade image raster raster_bwd silhouette camera meshreg points pointmesh knn baselines diffuse glossy glossy_bwd resample rotate metrics lights visibility texture splitsum"
case " $units " in
  *" $1 "*) ;;
  *) echo "usage: $0 {${units// /|}} OUT.s [hipcc flags]" >&2; exit 2 ;;
esac
hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -mllvm -amdgpu-spill-vgpr-to-agpr=0 -I../../include "${@:3}" -S --cuda-device-only "reni_tu_$1.hip" -o "$out"
