"""The reference-side adapters (vermilion_amd/adapter/*.cpp) are C++ that a Vermilion maintainer
compiles inside Vermilion.  Their syntax + type check against Vermilion's own headers needs a Vermilion
checkout, which the repository does not hold: it is `tools/adapter_check.sh <Vermilion>/core` (type-only
GLM / Assimp stand-ins in tests/stubs/, see its README).  The mesh walk itself runs in
tests/test_adapter_flatten.py."""
import glob
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADAPTERS = sorted(glob.glob(os.path.join(ROOT, "vermilion_amd", "adapter", "*.cpp")))


def test_adapters_exist():
    assert any(a.endswith("HipPathTracer.cpp") for a in ADAPTERS)
