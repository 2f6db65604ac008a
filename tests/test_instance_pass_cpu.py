"""What the four instance-table kernels share (``csrc/kernels/instance_pass.h``), as far as it shows without
a GPU: one chunk geometry, and the identities that tie their results together, on the reference path."""
import pytest

from _instance_pass_cases import PATTERNS, SHAPES, check_identities
from featurenet_amd import _native


def test_the_kernels_share_one_chunk_geometry():
    if not _native.kernels_available():
        pytest.skip("_C not built")
    K = _native.kernels()
    assert tuple(K.access_chunk()) == tuple(K.edt_chunk()) == tuple(K.overlap_chunk()) == (4096, 512)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=["under-a-wave", "two-chunks"])
def test_identities_hold_on_the_reference_path(shape, N, pattern):
    check_identities(pattern, N, shape, "cpu")
