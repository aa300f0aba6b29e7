"""Self-test of tests/buffer_checks.py on CPU tensors: a planted one-element overwrite is reported wherever it lands, a planted
change to an input is reported, and every offset gives exactly the address alignment it states."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from tests import buffer_checks as bc  # noqa: E402

CPU = torch.device("cpu")
DTYPES = [torch.float32, torch.int32, torch.int16]


def plant(t, index, value):
    t[index] = value


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_fresh_buffer_passes_and_holds_the_sentinel(dtype):
    buf = bc.carve(CPU, dtype, 1000, 3)
    bc.check_bands(buf)
    want = bc.SENTINEL16 if dtype == torch.int16 else bc.SENTINEL32
    assert (bc.bits(buf.region) == want).all() and buf.region.numel() == 1000 + 2 * bc.GUARD
    assert buf.view.numel() == 1000 and buf.view.is_contiguous() and buf.shaped(10, 100).data_ptr() == buf.view.data_ptr()
    if dtype == torch.float32:
        assert np.isnan(buf.host()).all()
    with pytest.raises(AssertionError, match="1000 element"):
        bc.check_all_written(buf)
    buf.view.zero_()
    assert not bc.check_all_written(buf).any()


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("where", ["front-last", "back-first", "front-far", "back-far"])
def test_one_planted_overwrite_is_reported(dtype, where):
    n = 777
    buf = bc.carve(CPU, dtype, n, 1)
    side, index, rel = {"front-last": ("front", bc.GUARD - 1, -1), "back-first": ("back", 0, n),
                        "front-far": ("front", 0, -bc.GUARD), "back-far": ("back", bc.GUARD - 1, n + bc.GUARD - 1)}[where]
    plant(buf.front() if side == "front" else buf.back(), index, 1)
    with pytest.raises(AssertionError) as e:
        bc.check_bands(buf, "planted")
    msg = str(e.value)
    assert f"{side} band: 1 element(s) changed" in msg and f"index {rel} " in msg and "planted" in msg
    assert ("front" if side == "back" else "back") + " band" not in msg


def test_stray_zero_and_stray_default_nan_count_as_overwrites():
    for value in (0.0, float("nan"), -0.0):
        buf = bc.carve(CPU, torch.float32, 64, 0)
        plant(buf.back(), 5, value)
        assert "back band: 1 element(s) changed, the first at index 69 " in bc.band_report(buf)
    # an input's NaN bands: a plain 0.0, and the sentinel NaN as well, differ from the quiet NaN they were filled with
    x = bc.carve_input(CPU, np.arange(64, dtype=np.float32), 1)
    assert (bc.bits(x.front()) == bc.QNAN32).all() and np.array_equal(x.host(), np.arange(64, dtype=np.float32))
    bc.check_bands(x)
    x.front().view(torch.int32)[-2] = bc.SENTINEL32
    assert "front band: 1 element(s) changed, the first at index -2 " in bc.band_report(x)
    i16 = bc.carve(CPU, torch.int16, 64, 0)
    plant(i16.front(), 7, 0)
    assert f"index {7 - bc.GUARD} " in bc.band_report(i16)


@pytest.mark.parametrize("dtype,which", [(np.float32, "nan"), (np.int16, "max"), (np.int16, "min"), (np.int32, "max"),
                                         (np.int32, "min")])
def test_planted_input_change_is_reported(dtype, which):
    data = (np.arange(500) % 97).astype(dtype)
    x = bc.carve_input(CPU, data, 2, which=which)
    if which != "nan":
        lim = np.iinfo(dtype).max if which == "max" else np.iinfo(dtype).min
        assert (x.front() == lim).all() and (x.back() == lim).all()
    snap = bc.snapshot(x)
    bc.check_untouched(x, snap)
    bc.check_bands(x)
    plant(x.view, 123, 99)
    with pytest.raises(AssertionError, match=r"1 element\(s\) changed, the first at index 123 "):
        bc.check_untouched(x, snap)
    bc.check_bands(x)                                   # the bands themselves are whole
    x.view[123] = float(data[123])
    bc.check_untouched(x, snap)
    plant(x.back(), 0, 1)
    with pytest.raises(AssertionError, match="first at index 500 "):
        bc.check_untouched(x, snap)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_every_offset_gives_exactly_its_alignment(dtype):
    size = torch.empty(0, dtype=dtype).element_size()
    for offset in (0, 1, 2, 3, 4, 5, 7, 8, 16, 63, 64):
        for numel in (1, 255, 4096):
            buf = bc.carve(CPU, dtype, numel, offset)
            assert buf.view.data_ptr() % bc.ALIGN == (offset * size) % bc.ALIGN, (offset, numel)
            assert buf.front().numel() == bc.GUARD and buf.back().numel() == bc.GUARD
            assert buf.back().data_ptr() == buf.view.data_ptr() + numel * size
    assert bc.carve(CPU, torch.float32, 10, 1).view.data_ptr() % 8 == 4
    assert bc.carve(CPU, torch.int16, 10, 1).view.data_ptr() % 4 == 2
    assert bc.carve(CPU, torch.int16, 10, 2).view.data_ptr() % 8 == 4
    assert bc.carve(CPU, torch.int16, 10, 4).view.data_ptr() % 16 == 8


def test_overlap_cases_share_one_allocation():
    for numel, out_numel in ((64, 64), (1000, 500), (100, 300)):
        cases = bc.overlap_cases(numel, out_numel, dtype=torch.int32)
        assert len(cases) == 3
        starts = []
        for a, b in cases:
            assert a.numel() == numel and b.numel() == out_numel and a.is_contiguous() and b.is_contiguous()
            assert a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()
            starts.append((b.data_ptr() - a.data_ptr()) // 4)
            assert (bc.bits(a) == bc.SENTINEL32).all() and (bc.bits(b) == bc.SENTINEL32).all()
        assert starts[0] == 0 and starts[1] == 1 and numel - numel // 4 <= starts[2] < numel
