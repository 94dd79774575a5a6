#!/bin/bash
# usage: tools/kres.sh file.hip [filter]  -- VGPR / spill / scratch / LDS per kernel (mangled name, then the figures: c++filt does not know __bf16)
cd "$(dirname "$0")/../prot2text-v2-esm3_amd/csrc"
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=on -mllvm -amdgpu-mfma-vgpr-form=1 \
  -Rpass-analysis=kernel-resource-usage -c "$1" -o /tmp/kres.o 2>&1 | sed 's/ \[-Rpass-analysis=kernel-resource-usage\]$//' | \
  awk '/Function Name:/{n=$NF} / VGPRs:/{v=$NF} /VGPRs Spill:/{sp=$NF} /ScratchSize/{sc=$NF} /LDS Size/{print n, "vgpr="v, "spill="sp, "scratch="sc, "lds="$NF}' | \
  grep -E "${2:-.}"
