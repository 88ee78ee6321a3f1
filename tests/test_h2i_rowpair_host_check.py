"""tests/h2i_rowpair_host_check.cpp: the row-pair geometry of trunk_kernel_h2i<128, 4, 3> checked on
the CPU from csrc/nn/rowpair.h's own functions -- the (tile set, tile, lane) -> (board, position) map is
a bijection, the skipped (set, tile, tap) are exactly the tiles wholly off the board, every B-fragment
read lies in its board's image or zero area and each ds_read_b128 lane group hits 16 distinct slots.
Built with -fsanitize=address,undefined (CPU only)."""
from test_fp32_mode import _run_sanitised


def test_rowpair_host_check_sanitised(tmp_path):
    p = _run_sanitised(tmp_path, "h2i_rowpair_host_check")
    assert p.returncode == 0, p.stdout[-4000:]
    for text in ("map: 128 positions", "skipped (set, tile, tap): 6 of 72", "conflict-free", "LDS per workgroup: 79200 B",
                 "h2i row-pair geometry: ok"):
        assert text in p.stdout, text
