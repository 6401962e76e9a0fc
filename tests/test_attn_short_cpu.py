"""CPU: the LDS footprint of the attention launch, by the library's host-only export (as_relpos_attention_image_lds_bytes).  The
short-sequence form (max_len <= 64) exists so that three workgroups share a CU's 160 KB of LDS -- a C3 launch of 192 members x 4 heads
is then resident in one round; this holds the footprint without a GPU.  Past 64 tokens the general form's size comes back."""
import pytest

from artspeech_amd import _lib

CU_LDS = 160 * 1024
# the general form (four waves): two 32 KB K tiles, the 32 KB V tile, the Ek operand with all 32 rows (16 KB), Ev^T (8 KB), Rk / Pb
GENERAL = (2 * 2048 + 2048 + 1024 + 512) * 16 + 4 * (128 * 9 + 128 * 16)


@pytest.mark.parametrize("max_len", [1, 32, 40, 64])
def test_three_short_workgroups_fit_a_cu(max_len):
    n = _lib.lib().as_relpos_attention_image_lds_bytes(max_len)
    assert n > 0 and 3 * n <= CU_LDS, (max_len, n)


def test_general_form_past_64_tokens():
    L = _lib.lib()
    assert L.as_relpos_attention_image_lds_bytes(65) == GENERAL == 135680
    assert L.as_relpos_attention_image_lds_bytes(1024) == GENERAL
    assert L.as_relpos_attention_image_lds_bytes(0) == 0 and L.as_relpos_attention_image_lds_bytes(-3) == 0
