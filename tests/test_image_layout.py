"""Where the image-space passes keep what they share: the Python classes in vermilion_amd/image.py, the device layer in
vmx_image.inc, the host argument layer in api_image.inc.  No GPU, no library."""
import pathlib
import re

import vermilion_amd as va
import vermilion_amd.image
import vermilion_amd.scene

CSRC = pathlib.Path(__file__).resolve().parent.parent / "vermilion_amd" / "csrc"


def test_the_handle_classes_are_one_object_under_every_import_path():
    for name in ("Filter", "Upsample", "Temporal"):
        cls = getattr(va.image, name)
        assert cls.__module__ == "vermilion_amd.image"
        assert getattr(va, name) is cls and getattr(va.scene, name) is cls


def test_editing_the_shared_device_layer_rebuilds_the_library():
    src = re.search(r"^SRC := (.*)$", (CSRC / "Makefile").read_text(), re.M).group(1).split()
    assert "vmx_image.inc" in src


def test_every_create_goes_through_the_shared_handle_check():
    for part in ("api_filter.inc", "api_temporal.inc", "api_upsample.inc"):
        text = (CSRC / part).read_text()
        assert "image_handle_checks(" in text, part
        assert '"image too large"' not in text, part
    assert '"image too large"' in (CSRC / "api_image.inc").read_text()
