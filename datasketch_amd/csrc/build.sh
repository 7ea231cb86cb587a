#!/usr/bin/env bash
# Build libmhx.so for gfx950 (MI355X) in-tree: datasketch_amd/libmhx.so
# hipcc cross-compiles without a GPU.  -ffp-contract=off: the weighted path must not fuse a*b+c.
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
OUT="${HERE}/../libmhx.so"
OBJ="${MHX_OBJ_DIR:-${HERE}/../../build/mhx}"
mkdir -p "${OBJ}"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
FLAGS=(--offload-arch=gfx950 -O3 -std=c++17 -fPIC -fvisibility=hidden -ffp-contract=off
       -I"${HERE}/../../include" -I"${HERE}" -Wall -Wno-unused-function)
pids=()
for src in mhx_api minhash_kernels weighted_kernels pack_kernels sha1_kernels xxh_kernels lsh_kernels lsh_index_kernels lsh_forest_kernels lsh_query_kernels jaccard_kernels jaccard_topk_kernels weighted_jaccard_kernels hll_kernels bloom_kernels cc_kernels words_kernels overlap_kernels comm; do
  if [[ ! -f "${OBJ}/${src}.o" || "${HERE}/${src}.hip" -nt "${OBJ}/${src}.o" \
        || "${HERE}/mhx_internal.h" -nt "${OBJ}/${src}.o" || "${HERE}/jaccard_tile.h" -nt "${OBJ}/${src}.o" || "${HERE}/jaccard_tile_count.inc" -nt "${OBJ}/${src}.o" || "${HERE}/band_digest.h" -nt "${OBJ}/${src}.o" || "${HERE}/device_scan.h" -nt "${OBJ}/${src}.o" || "${HERE}/window_walk.h" -nt "${OBJ}/${src}.o" || "${HERE}/../../include/mhx.h" -nt "${OBJ}/${src}.o" || "${HERE}/../../include/mhx_weighted_jaccard.h" -nt "${OBJ}/${src}.o" ]]; then
    "${HIPCC}" "${FLAGS[@]}" -c "${HERE}/${src}.hip" -o "${OBJ}/${src}.o" &
    pids+=($!)
  fi
done
for p in "${pids[@]:-}"; do [[ -n "${p}" ]] && wait "${p}"; done
"${HIPCC}" --offload-arch=gfx950 -shared -fPIC -o "${OUT}" "${OBJ}"/mhx_api.o "${OBJ}"/minhash_kernels.o \
  "${OBJ}"/weighted_kernels.o "${OBJ}"/pack_kernels.o "${OBJ}"/sha1_kernels.o "${OBJ}"/xxh_kernels.o "${OBJ}"/lsh_kernels.o "${OBJ}"/lsh_index_kernels.o "${OBJ}"/lsh_forest_kernels.o "${OBJ}"/lsh_query_kernels.o "${OBJ}"/jaccard_kernels.o "${OBJ}"/jaccard_topk_kernels.o "${OBJ}"/weighted_jaccard_kernels.o "${OBJ}"/hll_kernels.o "${OBJ}"/bloom_kernels.o "${OBJ}"/cc_kernels.o "${OBJ}"/words_kernels.o "${OBJ}"/overlap_kernels.o "${OBJ}"/comm.o -ldl
echo "built ${OUT}"
# CPython helper that packs Python byte tokens (host glue, plain C)
PYINC="$(python3 -c 'import sysconfig; print(sysconfig.get_paths()["include"])')"
gcc -O2 -shared -fPIC -Wall -I"${PYINC}" "${HERE}/pack_module.c" -o "${HERE}/../_mhxpack.so"
echo "built ${HERE}/../_mhxpack.so"
