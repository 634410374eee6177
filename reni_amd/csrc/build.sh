#!/bin/bash
# Build libreni_hip.so for gfx950 (cross-compiles without a GPU).  Usage: build.sh [extra hipcc flags]
# The translation units reni_tu_*.hip are compiled in parallel (see the header of reni_device.inc).
set -e
cd "$(dirname "$0")"
mkdir -p ../lib _build
# -amdgpu-spill-vgpr-to-agpr=0: the training kernel owns the AGPRs by hand (see mfma_bf16_agpr_tile)
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -mllvm -amdgpu-spill-vgpr-to-agpr=0 -I../../include"
pids=()
for tu in core main_f32 main_bf16 film_f32 film_bf16 train_film wide shade image raster raster_bwd silhouette camera meshreg points pointmesh knn baselines diffuse glossy glossy_bwd resample rotate metrics lights visibility texture splitsum; do
  hipcc $FLAGS "$@" -c reni_tu_$tu.hip -o _build/$tu.o &
  pids+=($!)
done
for p in "${pids[@]}"; do wait "$p"; done
hipcc --offload-arch=gfx950 -shared -fPIC _build/core.o _build/main_f32.o _build/main_bf16.o _build/film_f32.o _build/film_bf16.o _build/train_film.o _build/wide.o _build/shade.o _build/image.o _build/raster.o _build/raster_bwd.o _build/silhouette.o _build/camera.o _build/meshreg.o _build/points.o _build/pointmesh.o _build/knn.o _build/baselines.o _build/diffuse.o _build/glossy.o _build/glossy_bwd.o _build/resample.o _build/rotate.o _build/metrics.o _build/lights.o _build/visibility.o _build/texture.o _build/splitsum.o -o ../lib/libreni_hip.so
