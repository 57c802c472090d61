#!/bin/bash
# Developer builds of csrc/block.hip next to the product library, selected with ESPNET_AMD_LIB=... (espnet_amd/lib.py):
#   espnet_amd/lib/dbg/lib_nt.so      -DEM_BLOCK_NO_TOUCH=1                   (no L2 warm-up)
#   espnet_amd/lib/dbg/lib_fine.so    -DEM_BLOCK_FINE=1                       (EM_BLOCK_STAMPS=1 prints sub-stage stamps of all four waves)
#   espnet_amd/lib/dbg/lib_finent.so  -DEM_BLOCK_FINE=1 -DEM_BLOCK_NO_TOUCH=1
#   espnet_amd/lib/dbg/lib_<d>.so     -DEM_BLOCK_DBG=<d>                      (bits: 1 no MFMA / epilogue work; the attention phase: 128 no
#                                                                              exponentials, 256 no rel-shift scratch round trip, 512 the
#                                                                              operand requests of tile 0 only; sums combine)
#   espnet_amd/lib/dbg/lib_ffn<d>.so  csrc/ffn_rows.hip -DEM_FFN_DBG=<d>      (bits: 1 no MFMAs, 2 no weight requests, 4 no LDS operand reads,
#                                                                              8 cycle stamps)
# The <d> builds give wrong results by design: timing only.  The A/B variants of earlier rounds (lib_v<n>.so) are no longer in
# the source: HISTORY.md section H.   usage: bash tools/build_block_variants.sh nt fine 1 128 ffn8
set -eu
cd "$(dirname "$0")/.."
python -m espnet_amd.build >/dev/null
mkdir -p espnet_amd/lib/dbg
objs=$(ls espnet_amd/lib/*.o | grep -v "/block.o")
for v in "$@"; do
  case "$v" in
    ffn*)
      o2=$(ls espnet_amd/lib/*.o | grep -v "/ffn_rows.o")
      /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-gpu-rdc -Wno-unused-result -DEM_FFN_DBG=${v#ffn} \
        -Iinclude -Iespnet_amd/csrc -c espnet_amd/csrc/ffn_rows.hip -o espnet_amd/lib/dbg/ffn_rows_$v.o 2>/dev/null
      /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -pthread -o espnet_amd/lib/dbg/lib_$v.so $o2 espnet_amd/lib/dbg/ffn_rows_$v.o
      rm -f espnet_amd/lib/dbg/ffn_rows_$v.o
      echo "built espnet_amd/lib/dbg/lib_$v.so"; continue ;;
    nt) def="-DEM_BLOCK_NO_TOUCH=1" ;;
    finent) def="-DEM_BLOCK_FINE=1 -DEM_BLOCK_NO_TOUCH=1" ;;
    fine) def="-DEM_BLOCK_FINE=1" ;;
    [0-9]*) def="-DEM_BLOCK_DBG=$v" ;;
    *) echo "unknown build: $v" >&2; exit 2 ;;
  esac
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-gpu-rdc -Wno-unused-result -mllvm -amdgpu-mfma-vgpr-form \
    $def -Iinclude -Iespnet_amd/csrc -c espnet_amd/csrc/block.hip -o espnet_amd/lib/dbg/block_$v.o 2>/dev/null
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -pthread -o espnet_amd/lib/dbg/lib_$v.so $objs espnet_amd/lib/dbg/block_$v.o
  rm -f espnet_amd/lib/dbg/block_$v.o
  echo "built espnet_amd/lib/dbg/lib_$v.so"
done
