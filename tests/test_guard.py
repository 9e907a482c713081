"""CPU self-test of the guard-band helpers (tests/guard.py) that tests/test_hip_bounds.py relies on: each kind of stray store must be caught
and located, a store inside the view must not be, and poisoned inputs must hold their poison outside the view."""
import pytest
import torch

import guard


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16, torch.uint8, torch.int16, torch.int32, torch.float64])
def test_check_catches_every_kind_of_stray_store(dtype):
    rows, width, ld = 5, 12, 20
    g = guard.guarded((rows, width), dtype, ld=ld, guard_rows=3, device="cpu")
    assert g.view.stride() == (ld, 1) and (g.front * g.nbytes) % 16 == 0
    g.check()
    g.view.copy_(torch.arange(rows * width).reshape(rows, width).to(dtype))  # stores inside the view are the kernel's business
    g.check()
    s = guard.SENTINEL[dtype]
    cases = {
        "one past a row's width": (g.front + 2 * ld + width, (2, width), "in the row padding"),
        "last element of a row's pitch padding": (g.front + 3 * ld + ld - 1, (3, ld - 1), "in the row padding"),
        "one before the view's start": (g.front - 1, (-1, ld - 1), "before the view"),
        "first element of the front guard": (0, None, "before the view"),
        "one after the view's end": (g.front + (rows - 1) * ld + width, (rows - 1, width), "behind the view"),
        "one whole row behind the view": (g.front + rows * ld, (rows, 0), "behind the view"),
        "last element of the back guard": (g.total - 1, None, "behind the view"),
    }
    for name, (flat, rc, where) in cases.items():
        saved = g.ibase[flat].clone()
        g.ibase[flat] = guard._signed(s ^ 1, g.nbytes)  # one bit: for the float types a change of the NaN payload only
        if dtype.is_floating_point:
            assert torch.isnan(g.base[flat]), name
        with pytest.raises(AssertionError) as e:
            g.check()
        msg = str(e.value)
        assert where in msg and "1 element(s)" in msg, (name, msg)
        if rc is not None:
            assert f"(row {rc[0]}, column {rc[1]})" in msg, (name, msg)
        g.ibase[flat] = saved
        g.check()


def test_check_catches_a_store_of_another_nan_and_of_zero():
    g = guard.guarded((4, 8), torch.float32, guard_rows=1, device="cpu")
    g.base[g.front + 32] = float("nan")  # the canonical NaN is not the sentinel's NaN
    with pytest.raises(AssertionError, match="behind the view"):
        g.check()
    g = guard.guarded((4, 8), torch.float16, device="cpu")
    g.base[g.front - 1] = 0.0
    with pytest.raises(AssertionError, match="before the view"):
        g.check()


def test_higher_rank_views_and_the_second_sentinel():
    view, check = guard.guarded_out((3, 4, 10), torch.uint8, ld=16, device="cpu")
    assert view.stride() == (64, 16, 1)
    view.fill_(7)
    check()
    view2, check2 = guard.guarded_out((3, 4, 10), torch.uint8, ld=16, device="cpu", sentinel=guard.ALT_SENTINEL[torch.uint8])
    assert int(view2[0, 0, 0]) == 0x5A
    view2.as_strided((1,), (1,), view2.storage_offset() + 10).fill_(0x5A)  # a stray store of the sentinel's own value goes unseen ...
    check2()
    view.as_strided((1,), (1,), view.storage_offset() + 10).fill_(0x5A)    # ... but not under the other sentinel
    with pytest.raises(AssertionError, match=r"\(row 0, column 10\)"):
        check()


def test_init_and_unwritten_view_elements():
    init = torch.randn(6, 8)
    view, check = guard.guarded_out((6, 8), torch.float32, ld=12, device="cpu", init=init)
    assert torch.equal(view, init)
    check()
    view, _ = guard.guarded_out((6, 8), torch.float32, device="cpu")
    assert torch.isnan(view).all()  # an element a kernel should write and does not stays a NaN


@pytest.mark.parametrize("dtype,poison", [(torch.float32, None), (torch.float16, None), (torch.bfloat16, None), (torch.uint8, 255), (torch.int16, -1)])
def test_poisoned_in_holds_poison_outside_the_view(dtype, poison):
    data = (torch.arange(5 * 24).reshape(5, 24) % 50).to(dtype)
    v = guard.poisoned_in(data, ld=40, guard_rows=2)
    assert torch.equal(v, data) and v.stride() == (40, 1)
    assert (v.storage_offset() * v.element_size()) % 16 == 0
    flat = torch.as_strided(v, (v.untyped_storage().nbytes() // v.element_size(),), (1,), 0)
    o = v.storage_offset()
    for part in (flat[o + 24:o + 40], flat[:o], flat[o + 4 * 40 + 24:]):
        if dtype.is_floating_point:
            f = part.float()
            big = float(torch.tensor(65504.0).to(dtype).float())
            assert torch.isnan(f).any() and (f == float("inf")).any() and (f == -float("inf")).any() and (f == big).any()
        else:
            assert (part == poison).all()
