#!/bin/bash
# Syntax + type check of the reference-side adapters (vermilion_amd/adapter/*.cpp) against the headers of a Vermilion
# checkout, with the type-only GLM / Assimp stand-ins of tests/stubs/.   bash tools/adapter_check.sh <Vermilion>/core
set -e -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
REF=${1:?usage: tools/adapter_check.sh <path of the core/ directory of a Vermilion checkout>}
for src in "$R"/vermilion_amd/adapter/*.cpp; do
  g++ -std=c++17 -fsyntax-only -Wall -Wextra -Werror -I "$R/tests/stubs" -I "$REF" -I "$R/include" \
    -I "$R/vermilion_amd/adapter" "$src"
  echo "adapter check ok: $(basename "$src")"
done
