"""The four instance-table kernels (``ccl_stats``, ``overlap_pairs``, ``access_stats``, ``edt_stats``) on one
volume on the GPU, tied to each other and to the CPU oracle: they share ``csrc/kernels/instance_pass.h``, and
what one of them counts the others must count too.  Every comparison is ``torch.equal``.  The kernels'
branches are walked path by path in ``test_ccl_gpu.py``, ``test_overlap_gpu.py``, ``test_access_gpu.py`` and
``test_edt_gpu.py``."""
import pytest

pytestmark = pytest.mark.gpu

from _instance_pass_cases import PATTERNS, SHAPES, check_identities  # noqa: E402


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=["under-a-wave", "two-chunks"])
def test_the_four_kernels_agree(shape, N, pattern):
    check_identities(pattern, N, shape, "cuda")
