"""The red-zone helpers of tests/_guards.py on CPU tensors: a test that relies on a sentinel is only as good as the sentinel check."""
import pathlib
import re

import pytest
import torch

from tests._guards import GUARD, _guarded, _guards_intact, scratch, scratch_sentinel

NAN = float("nan")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("fill", [NAN, -7.0])
@pytest.mark.parametrize("shape", [(1,), (3, 5), (2, 3, 7)])
def test_guarded_view_aliases_the_buffer_between_two_intact_bands(dtype, fill, shape):
    t = torch.arange(1, 1 + torch.Size(shape).numel(), dtype=dtype).view(shape)
    buf, view = _guarded(t, fill)
    assert buf.numel() == 2 * GUARD + t.numel() and view.shape == t.shape and torch.equal(view, t)
    assert view.data_ptr() == buf.data_ptr() + GUARD * buf.element_size()
    assert _guards_intact(buf, fill)
    view.mul_(2)                                           # writes through the view land in the buffer, not in the bands
    assert torch.equal(buf[GUARD:GUARD + t.numel()].view(shape), 2 * t) and _guards_intact(buf, fill)


# (a NaN written into a NaN band is indistinguishable by value: NaN bands surround inputs, which kernels only read)
@pytest.mark.parametrize("fill,value", [(NAN, 0.0), (NAN, 1.0), (NAN, float("inf")), (-7.0, 0.0), (-7.0, 1.0), (-7.0, NAN), (-7.0, float("inf")),
                                        (-7.0, 7.0)])
@pytest.mark.parametrize("where", ["one before", "one after", "first of the low band", "last of the high band"])
def test_a_single_foreign_element_in_either_band_is_detected(fill, where, value):
    buf, view = _guarded(torch.zeros(5), fill)
    idx = {"one before": GUARD - 1, "one after": GUARD + 5, "first of the low band": 0, "last of the high band": buf.numel() - 1}[where]
    buf[idx] = value
    assert not _guards_intact(buf, fill)


def test_nan_sentinels_compare_as_sentinels_and_finite_sentinels_reject_nan():
    buf, _ = _guarded(torch.zeros(3), NAN)
    assert _guards_intact(buf, NAN)                        # NaN != NaN must not read as "damaged"
    assert not _guards_intact(buf, -7.0)                   # ... and a NaN band is not a -7 band
    buf, _ = _guarded(torch.zeros(3), -7.0)
    assert _guards_intact(buf, -7.0) and not _guards_intact(buf, NAN) and not _guards_intact(buf, 7.0)
    buf[GUARD - 1] = torch.nextafter(torch.tensor(-7.0), torch.tensor(-8.0))     # one ulp off the sentinel
    assert not _guards_intact(buf, -7.0)


@pytest.mark.parametrize("dtype,fill", [(torch.float32, NAN), (torch.float32, 0.0), (torch.float64, NAN), (torch.float64, 0.0),
                                        (torch.uint8, 0xFF), (torch.uint8, 0)])
@pytest.mark.parametrize("nelem", [0, 1, 3, 7, 1025])
def test_scratch_has_exactly_the_requested_elements_aligned_between_sentinels(dtype, fill, nelem):
    buf, view = scratch(nelem, dtype, fill, device="cpu")
    sent = scratch_sentinel(dtype)
    assert view.numel() == nelem and view.dtype == dtype and buf.numel() == nelem + 2 * GUARD
    if nelem:                                              # (an empty view has no address)
        assert view.data_ptr() % 16 == 0
        assert view.data_ptr() == buf.data_ptr() + GUARD * buf.element_size()
    assert _guards_intact(buf, sent)
    if fill != fill:
        assert torch.isnan(view).all()
    else:
        assert (view == fill).all()
    assert (buf[:GUARD] == sent).all() and (buf[GUARD + nelem:] == sent).all()       # the bands touch the view: nothing in between
    view.fill_(1)                                          # a kernel that stays inside leaves the bands alone
    assert _guards_intact(buf, sent)
    buf[GUARD - 1] = 1                                     # one element before the view
    assert not _guards_intact(buf, sent)
    buf[GUARD - 1] = sent
    buf[GUARD + nelem] = 1                                 # one element after the view
    assert not _guards_intact(buf, sent)


def test_scratch_detects_a_nan_written_outside_a_nan_filled_interior():
    buf, view = scratch(6, torch.float32, NAN, device="cpu")
    assert _guards_intact(buf, scratch_sentinel(torch.float32))
    buf[GUARD + 6] = NAN                                   # what a reducer's stray NaN store would leave
    assert not _guards_intact(buf, scratch_sentinel(torch.float32))


def test_no_module_under_tests_imports_a_test_module():
    """helpers live in the `_*.py` modules: a test module is never a library, so an import error in one cannot take another down"""
    here = pathlib.Path(__file__).parent
    pat = re.compile(r"from tests\.test_|from tests import +test_|import tests\.test_")
    bad = [(p.name, i + 1) for p in sorted([*here.glob("*.py"), *here.glob("tools/*.py")]) for i, line in enumerate(p.read_text().splitlines()) if pat.search(line)]
    assert not bad, bad


def test_only_the_two_switch_tables_read_the_environment_and_the_docs_list_them():
    """no launcher latches a variable of its own: csrc/api.hip reads the environment for the library (VS_DBG_KEYS, csrc/vs_common.h) and
    videoseal_amd/switches.py for the Python side; INTEGRATION.md's table lists exactly the names of both"""
    root = pathlib.Path(__file__).parent.parent
    pkg = root / "videoseal_amd"
    c_files = [p for d in (pkg / "csrc", root / "include") for p in d.rglob("*") if p.suffix in (".hip", ".h", ".hpp", ".c", ".cpp")]
    assert len(c_files) > 20
    assert [str(p) for p in c_files if p.name != "api.hip" and "getenv" in p.read_text()] == []
    assert "getenv" in (pkg / "csrc" / "api.hip").read_text()
    py = [p for p in pkg.rglob("*.py") if p.name != "switches.py"]
    assert len(py) > 10
    assert [str(p) for p in py if re.search(r"os\.environ|os\.getenv|\benviron\b|\bgetenv\b", p.read_text())] == []
    from videoseal_amd import switches
    rows = re.findall(r'^\s*X\((\w+), (?:"(\w+)"|nullptr), ', (pkg / "csrc" / "vs_common.h").read_text(), re.M)
    assert len(rows) >= 21
    names = {env for _, env in rows if env} | set(switches.REGISTRY)
    assert all(re.fullmatch(r"(VIDEOSEAL|VS)_[A-Z0-9_]+", n) for n in names)
    doc = (root / "INTEGRATION.md").read_text()
    table = doc[doc.index("| variable | key (`vs_debug_key` name) |"):doc.index("Other handles:")]
    cells = [re.split(r"(?<!\\)\|", line)[1:3] for line in table.splitlines()[2:] if line.startswith("|")]
    listed = {m.group(1) for var, _ in cells for m in [re.match(r" `((?:VIDEOSEAL|VS)_[A-Z0-9_]+)", var)] if m}
    assert listed == names
    assert [key.strip() for _, key in cells if key.strip() != "-"] == [f"{k} `{name}`" for k, (name, _) in enumerate(rows)]      # every key, in order
