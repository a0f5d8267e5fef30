"""The workspace slice of the HBM-resident family (layout_big_workspace, through plo_cse_hbm_workspace_layout: host only, nothing
is allocated).  The kernels address everything in front of the pair table with 32-bit byte offsets, so the table must come last,
and a front region beyond 4 GiB must select the kernels with 64-bit offsets -- which the kernels' stated limits (32766 rows of
8192 entries, 32768 columns) do reach: the front region holds seven 4-byte arrays and one 8-byte array per entry, 36 bytes."""
import ctypes

LIM_ROWS, LIM_ROWLEN, LIM_COLS = 32766, 8192, 32768


def _layout(rows, nnz, ncmax, bits):
    from plinopt_amd import capi
    out = (ctypes.c_uint64 * 3)()
    capi.check(capi.lib().plo_cse_hbm_workspace_layout(rows, nnz, ncmax, bits, out))
    return out[0], out[1], out[2]


def test_table_comes_last_and_config5_is_narrow():
    front, slice_, wide = _layout(15096, 1257376, 32768, 24)
    assert wide == 0 and front <= 0xFFFFFFFF
    assert 36 * 1257376 <= front < 40 * 1257376 + (64 << 20)         # 36 bytes per entry, and the lists that do not grow with nnz
    assert slice_ == front + (8 << 24) and front % 256 == 0          # nothing behind the table
    # the refits multiply the table by up to 256: only the slice grows, the front region (and the choice of kernels) stays
    assert _layout(15096, 1257376, 32768, 30) == (front, front + (8 << 30), 0)


def test_stated_limits_take_the_wide_kernels():
    front, slice_, wide = _layout(LIM_ROWS, LIM_ROWS * LIM_ROWLEN, LIM_COLS, 30)
    assert front >= 36 * LIM_ROWS * LIM_ROWLEN > 1 << 32 and wide == 1
    assert slice_ == front + (8 << 30)


def test_wide_is_chosen_exactly_above_4_gib():
    n0 = (1 << 32) // 36                                            # entries at which 36 bytes each make 4 GiB
    seen = set()
    for nnz in range(n0 - (1 << 20), n0 + (1 << 17), 1 << 14):
        front, _, wide = _layout(LIM_ROWS, nnz, LIM_COLS, 30)
        assert wide == (1 if front > 0xFFFFFFFF else 0), (nnz, front, wide)
        seen.add(wide)
    assert seen == {0, 1}
