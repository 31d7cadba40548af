"""CPU tests of aic_pick_pixels' restatement (tests/pick_ref.py) and of its Python structures: the picker part against the host mirror's PixelPicker,
the unknown part on hand-made splat images with known answers, the arithmetic of g, and abi.py's structures against include/aic_hip.h."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from all_is_cubes_amd import _host as H
from all_is_cubes_amd import abi
from tests import pick_ref
from tests import reproject_ref as ref

ROOT = Path(__file__).resolve().parents[1]
VALID = np.array([0x3C00, 0x3800, 0x0001, 0x3C00], np.uint16)  # any texel with alpha 1.0


@pytest.mark.parametrize("w,h", [(1, 1), (2, 2), (3, 5), (64, 48)])
def test_picker_part_equals_the_mirrors_pixel_picker(w, h):
    order, central, cycle = abi.pixel_order(w, h)
    count = w * h
    assert central == min(pick_ref.CENTRAL_MAX, count // 4) and cycle == 2 * max(central, count - central)
    n = 2 * cycle
    want = H.PixelPicker(w, h).take(n)
    got, info = pick_ref.pick_list(count, order, n)
    assert got.dtype == np.uint32 and (got == want).all()
    assert info == {"n_unknown": 0, "next_cursor": n, "n_from_unknown": 0, "n_from_order": n}
    # from a cursor inside the sequence, and split into two calls
    a, ia = pick_ref.pick_list(count, order, 5, cursor=3)
    b, _ = pick_ref.pick_list(count, order, 4, cursor=ia["next_cursor"])
    assert (np.concatenate([a, b]) == want[3:12]).all()
    assert set(int(v) for v in got[:cycle]) == set(range(count)), "the first cycle covers every pixel"


def splat_image(w, h, unknown_pixels, texel=ref.MARKER):
    R = np.tile(VALID, (h, w, 1))
    for p in unknown_pixels:
        R[p // w, p % w] = texel
    return R


def test_hand_made_splat_images():
    w, h = 7, 5
    count = w * h
    order, central, _ = abi.pixel_order(w, h)
    assert central == 8
    rank_of = {int(p): r for r, p in enumerate(order)}
    # all valid: nothing unknown, the list is the picker's
    got, info = pick_ref.pick_list(count, order, 9, R=splat_image(w, h, []), max_unknown=9)
    assert info["n_unknown"] == 0 and info["n_from_unknown"] == 0 and (got == H.PixelPicker(w, h).take(9)).all()
    # all marker: the rank list is the order itself
    R = splat_image(w, h, range(count))
    got, info = pick_ref.pick_list(count, order, count + 2, R=R, max_unknown=count + 2)
    assert info == {"n_unknown": count, "next_cursor": 2, "n_from_unknown": count, "n_from_order": 2}
    assert (got[:count] == order).all() and list(got[count:]) == [order[0], order[central]]
    got, _ = pick_ref.pick_list(count, None, count, R=R, max_unknown=count)
    assert (got == np.arange(count)).all(), "row-major without an order"
    # one unknown pixel, at the last rank
    last = int(order[-1])
    got, info = pick_ref.pick_list(count, order, 3, R=splat_image(w, h, [last]), max_unknown=3)
    assert info["n_unknown"] == 1 and list(got) == [last, order[0], order[central]]
    # several: listed by rank, not by index
    some = [0, 17, 18, 34]
    got, info = pick_ref.pick_list(count, order, 4, R=splat_image(w, h, some), max_unknown=4)
    assert list(got) == sorted(some, key=rank_of.get) and info["n_unknown"] == 4
    # NaN alpha is unknown; alpha -0.5 exactly is unknown, the next f16 above it is not
    for alpha_bits, is_unknown in ((0x7E00, True), (0xFE00, True), (0xB800, True), (0xB7FF, False), (0x8000, False), (0xFC00, True)):
        texel = np.array([1, 2, 3, alpha_bits], np.uint16)
        got, info = pick_ref.pick_list(count, order, 1, R=splat_image(w, h, [12], texel), max_unknown=1)
        assert info["n_unknown"] == int(is_unknown), hex(alpha_bits)
        assert int(got[0]) == (12 if is_unknown else int(order[0]))
    # an order entry that is no pixel is never unknown and is written as it is by the picker part
    bad = order.copy()
    bad[0] = count + 5
    got, info = pick_ref.pick_list(count, bad, 2, R=splat_image(w, h, range(count)), max_unknown=1)
    assert info["n_unknown"] == count - 1 and list(got) == [order[1], count + 5]


def test_g_arithmetic():
    w, h = 7, 5
    count = w * h
    order, central, _ = abi.pixel_order(w, h)
    unknown_pixels = [3, 4, 10, 20, 21, 30]
    R = splat_image(w, h, unknown_pixels)
    ranks = pick_ref.rank_list(R, order)
    assert sorted(int(v) for v in ranks) == unknown_pixels
    nu = len(ranks)
    for skip, n, mx, g in ((0, 10, 10, 6), (0, 4, 10, 4), (0, 10, 2, 2), (3, 10, 10, 3), (3, 10, 2, 2), (nu, 10, 10, 0), (nu + 5, 10, 10, 0), (nu - 1, 10, 10, 1),
                           (2**40, 10, 10, 0), (0, 10, 0, 0)):
        assert pick_ref.taken(n, mx, nu, skip) == g
        got, info = pick_ref.pick_list(count, order, n, R=R, max_unknown=mx, skip_unknown=skip, cursor=7)
        assert info["n_from_unknown"] == g and info["n_from_order"] == n - g and info["next_cursor"] == 7 + n - g
        assert info["n_unknown"] == (nu if mx else 0)
        assert (got[:g] == ranks[skip:skip + g]).all()
        assert list(got[g:]) == [pick_ref.pick(7 + j, count, order) for j in range(n - g)]
    assert pick_ref.pick_list(count, order, 0, R=R, max_unknown=3)[1]["n_unknown"] == 0, "n = 0: nothing looked at"
    assert pick_ref.pick(2**64 - 1, count, order) == int(order[central + (2**63 - 1) % (count - central)])


def header_struct(name):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "aic_hip.h").read_text(), flags=re.S)
    body = re.search(r"typedef struct %s\s*\{(.*?)\}\s*%s\s*;" % (name, name), text, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype = decl.split()[0]
            fields += [(part.strip().split()[-1], ctype) for part in decl.split(",")]
    return fields


def test_structures_match_the_header():
    ctypes_of = {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "float": C.c_float}
    for cls, name, size in ((abi.PickDesc, "aic_pick_desc", 40), (abi.PickInfo, "aic_pick_info", 32)):
        want = [(field, ctypes_of[ctype]) for field, ctype in header_struct(name)]
        assert [(f[0], f[1]) for f in cls._fields_] == want, name
        assert C.sizeof(cls) == size, name
    assert abi.PickDesc.skip_unknown.offset == 16 and abi.PickDesc.cursor.offset == 24 and abi.PickDesc.flags.offset == 32
    assert abi.PickInfo.n_from_unknown.offset == 16 and abi.PickInfo.kernel_ms.offset == 24
    assert "aic_pick_pixels" in abi.ABI_SYMBOLS and hasattr(abi.load(), "aic_pick_pixels")
