"""What the seeded shape draw of tests/_product_loops.py (loop_fuzz_shapes) must contain, by arithmetic: no GPU needed.
tests/test_gpu_product_loops.py runs every drawn shape on each product loop; a change of the seed or of the draw that
loses one of these classes fails here."""
from _product_loops import FUZZ_F, FUZZ_M, FUZZ_N, FUZZ_RATE, FUZZ_ROWS, loop_fuzz_shapes, matrix_cores_take


def _blocks(s):
    return (s[2] * s[3] + 31) // 32


def _rows(s):
    return s[4] // s[2]


def _index_passes_rate(s):
    """The NCO sample index passes `rate` strictly inside one of the three buffers."""
    N, rate, M, F, L = s
    return any((c * L) % rate + L > rate and ((c + 1) * L) % rate != 0 for c in range(3))


def test_the_draw_is_seeded_and_every_shape_is_taken_by_the_matrix_cores():
    shapes = loop_fuzz_shapes()
    assert shapes == loop_fuzz_shapes() and len(shapes) == 36
    for N, rate, M, F, L in shapes:
        assert matrix_cores_take(M, F, L), (N, rate, M, F, L)
        assert FUZZ_F[0] <= F <= FUZZ_F[1] and M in FUZZ_M and rate in FUZZ_RATE and N in FUZZ_N
        assert L % M == 0 and max(F - 1, 1) <= L // M <= FUZZ_ROWS


def test_the_draw_holds_every_class_of_shape():
    shapes = loop_fuzz_shapes()
    classes = {
        "a window of one block": lambda s: _blocks(s) == 1,
        "a window of two blocks": lambda s: _blocks(s) == 2,
        "an odd block count of three or more": lambda s: _blocks(s) >= 3 and _blocks(s) % 2 == 1,
        "M * F no multiple of 32": lambda s: s[2] * s[3] % 32 != 0,
        "rows == F - 1": lambda s: _rows(s) == s[3] - 1,
        "at most 16 rows": lambda s: _rows(s) <= 16,
        "17 to 32 rows": lambda s: 17 <= _rows(s) <= 32,
        "more than 32 rows, no multiple of 16": lambda s: _rows(s) > 32 and _rows(s) % 16 != 0,
        "F of at least 6": lambda s: s[3] >= 6,
        "65 tones": lambda s: s[0] == 65,
        "at least 130 tones": lambda s: s[0] >= 130,
        "M >= rate": lambda s: s[2] >= s[1],
    }
    for name, holds in classes.items():
        assert any(holds(s) for s in shapes), name
    assert sum(_index_passes_rate(s) for s in shapes) >= 5


def test_the_pipelined_fuzz_shapes_hold_short_and_long_windows_and_several_tone_groups():
    """test_pipelined_fuzz runs the first 12: among them odd and even block counts and more than one wave of tones."""
    first = loop_fuzz_shapes()[:12]
    assert any(_blocks(s) % 2 for s in first) and any(_blocks(s) % 2 == 0 for s in first)
    assert any(s[0] > 64 for s in first) and any(_rows(s) > 32 for s in first)
