"""tests/footprint.py proved on the CPU: every injected fault is reported by the check named for it, and clean stand-ins pass.

The "kernels" here are plain torch functions of THIS module; the guard is told to treat this module as the package
(packages=(__name__,)) and to guard CPU tensors (any_device=True).  The out-of-bounds stores are `as_strided` views into
the guarded allocation: legal stores inside one allocation, exactly what a stray kernel store into a guard is."""
import pytest
import torch

from tests import footprint as fp

ME = (__name__,)


def _before(t, k=1):
    return t.as_strided((k,), (1,), t.storage_offset() - k)


def _after(t, k=1, skip=0):
    return t.as_strided((k,), (1,), t.storage_offset() + t.numel() + skip)


# ------------------------------------------------------------------ stand-in kernels (allocate like the hosts do)
def k_scale(x):                                   # clean elementwise op
    out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    torch.mul(x, 2.0, out=out)
    return out


def k_padded(x, n_pad, d_pad):                    # clean padded-layout writer: pads keep what zeros() put there
    n, d = x.shape
    buf = torch.zeros(n_pad, d_pad, dtype=x.dtype, device=x.device)
    buf[:n, :d] = x
    return buf


def k_store_before(x):
    out = k_scale(x)
    _before(out.view(-1)).fill_(3.0)
    return out


def k_store_after(x):
    out = k_scale(x)
    _after(out.view(-1)).fill_(3.0)
    return out


def k_store_row_past(x):
    out = k_scale(x)
    _after(out.view(-1), k=x.shape[-1], skip=0).fill_(3.0)
    return out


def k_writes_input(x):
    out = k_scale(x)
    x.view(-1)[0] = 7.0
    return out


def k_reads_scratch(x):
    ws = torch.empty(16, dtype=torch.float32, device=x.device)       # read before written
    return k_scale(x) + ws[3]


def k_reads_past_row(x):                          # reads one element past each row (but the last) of a strided view
    wide = x.as_strided((x.shape[0] - 1, x.shape[1] + 1), x.stride(), x.storage_offset())
    out = torch.empty(x.shape[0] - 1, dtype=x.dtype, device=x.device)
    torch.sum(wide, dim=1, out=out)
    return out


def k_bypass(x):
    buf = torch.empty_like(x)
    out = torch.zeros(x.shape, out=buf)                              # `out=`: not an allocation the wrapper understands
    return out + x


def _x(rows=5, cols=7):
    return torch.arange(rows * cols, dtype=torch.float32).view(rows, cols) / 8 + 1


def _run(kernel, fill=0xFF, **kw):
    with fp.guarded(fill, ME, any_device=True) as g:
        h = g.guard_input(_x(**kw), "x")
        return kernel(h.t)


# ------------------------------------------------------------------ the mechanism itself
def test_layout_alignment_fill_and_guard_size():
    with fp.guarded(0xFF, ME, any_device=True) as g:
        a = torch.empty(3, 5, dtype=torch.float16)
        b = torch.empty(300, 1000, dtype=torch.float32)
        c = torch.zeros((4, 4), dtype=torch.int32)
        d = torch.full((2, 3), 2.5)
        e = torch.ones(6, dtype=torch.float64)
        f = torch.empty_like(a)
        gg = a.new_zeros(2, 2)
        hh = a.new_full((3,), 4.0)
        i = torch.empty(0, 3, dtype=torch.float32)
        p = torch.empty_like(b.t())                       # permuted dense source: strides preserved
        n = torch.zeros_like(b[:, 0])                     # non-dense source: contiguous result
        assert len(g.records) == 11 and not g.bypassed
        for t in (a, b, c, d, e, f, gg, hh, p, n):
            assert t.data_ptr() % fp.ALIGN == 0
        assert a.shape == (3, 5) and a.dtype == torch.float16 and a.is_contiguous() and torch.isnan(a).all()
        assert torch.isnan(b).all() and torch.isnan(f).all() and f.shape == a.shape
        assert (c == 0).all() and (d == 2.5).all() and (e == 1).all() and (gg == 0).all() and (hh == 4).all()
        assert gg.dtype == hh.dtype == torch.float16 and i.shape == (0, 3)
        assert p.shape == (1000, 300) and p.stride() == (1, 1000) and n.is_contiguous() and (n == 0).all()
        ra, rb = g.records[0], g.records[1]
        assert ra.hi - ra.lo == 30 and ra.lo >= fp.GUARD_MIN and ra.base.numel() - ra.hi >= fp.GUARD_MIN
        assert rb.lo >= 256 * 4000 and rb.base.numel() - rb.hi >= 256 * 4000       # 256 rows of the tensor's own pitch
        # the back guard sits directly behind the last element
        assert ra.base.data_ptr() + ra.hi == a.data_ptr() + a.numel() * 2
    with fp.guarded(0x00, ME, any_device=True):
        z = torch.empty(4, dtype=torch.int32)
        assert (z == 0).all()
    with fp.guarded(0xFF, ME, any_device=True):
        assert (torch.empty(4, dtype=torch.int32) == -1).all()


def test_factories_are_restored_and_outsiders_pass_through():
    real = (torch.empty, torch.zeros_like, torch.Tensor.new_empty)
    with fp.guarded(0xFF, ("some_other_package",), any_device=True) as g:
        assert torch.empty is not real[0]
        t = torch.empty(4)                                # this module is not the package here: untouched
        assert not g.records and not g.bypassed and t.shape == (4,)
    assert (torch.empty, torch.zeros_like, torch.Tensor.new_empty) == real
    with pytest.raises(ZeroDivisionError):
        with fp.guarded(0xFF, ME, any_device=True):
            1 / 0
    assert (torch.empty, torch.zeros_like, torch.Tensor.new_empty) == real
    with fp.guarded(0xFF, ME) as g:                       # device mode: CPU allocations pass through
        torch.empty(4)
        assert not g.records and not g.bypassed


def test_guard_input_keeps_strides_and_poisons_the_gaps():
    big = torch.arange(60, dtype=torch.float32).view(5, 12)
    view = big[:, 2:9:2]                                  # strides (12, 2)
    with fp.guarded(0xFF, ME, any_device=True) as g:
        h = g.guard_input(view, "view")
        assert h.t.stride() == view.stride() and torch.equal(h.t, view) and h.t.data_ptr() % fp.ALIGN == 0
        assert torch.isnan(h.t.as_strided((5, 3), (12, 2), h.t.storage_offset() + 1)).all()      # the elements between the view's are poison
        h.assert_unchanged()


# ------------------------------------------------------------------ clean stand-ins pass
def test_clean_elementwise_passes():
    out = fp.hold(lambda g: k_scale(g.guard_input(_x(), "x").t), ME, any_device=True)
    assert torch.equal(out, _x() * 2)


def test_clean_padded_writer_passes_and_keeps_its_pads():
    out = fp.hold(lambda g: k_padded(g.guard_input(_x(), "x").t, 8, 16), ME, any_device=True)
    assert torch.equal(out[:5, :7], _x()) and (out[5:] == 0).all() and (out[:, 7:] == 0).all()


# ------------------------------------------------------------------ each injected fault is reported by its own check
def test_store_one_element_before_is_reported():
    with pytest.raises(fp.FootprintError, match=r"empty allocated at .*test_footprint_cpu.py:\d+: front guard damaged, 4 bytes, "
                                                r"offsets -4 \.\. -1 "):
        _run(k_store_before)


def test_store_one_element_after_is_reported():
    with pytest.raises(fp.FootprintError, match=r"back guard damaged, 4 bytes, offsets 0 \.\. 3 "):
        _run(k_store_after)


def test_store_a_full_row_past_the_end_is_reported():
    with pytest.raises(fp.FootprintError, match=r"back guard damaged, 28 bytes, offsets 0 \.\. 27 "):
        _run(k_store_row_past)
    with fp.guarded(0xFF, ME, any_device=True) as g:      # the report, structured: exactly one guard, of the output
        h = g.guard_input(_x(), "x")
        k_store_row_past(h.t)
        found = g.damaged()
        g.records.clear()                                 # (reported above; leave the block quietly)
    assert len(found) == 1 and "back guard" in found[0]


def test_write_into_const_input_is_reported():
    with pytest.raises(fp.FootprintError, match=r"const operand 'input x' .* was written: \d+ bytes differ"):
        _run(k_writes_input)
    with fp.guarded(0x00, ME, any_device=True) as g:
        h = g.guard_input(_x(), "x")
        k_writes_input(h.t)
        with pytest.raises(fp.FootprintError, match="const operand x"):
            h.assert_unchanged()
        assert h.changed_bytes() > 0 and len(g.written_inputs()) == 1 and not g.damaged()
        g.records.clear()
    with fp.guarded(0x00, ME, any_device=True) as g:      # a documented in-place operand is not held to its snapshot
        h = g.guard_input(_x(), "x", const=False)
        k_writes_input(h.t)


def test_result_depending_on_empty_contents_is_reported():
    with pytest.raises(fp.FootprintError, match=r"results depend on the contents of torch.empty scratch"):
        fp.hold(lambda g: k_reads_scratch(g.guard_input(_x(), "x").t), ME, any_device=True)


def test_out_of_bounds_read_next_to_an_input_is_reported():
    view = torch.ones(5, 12)[:, :7]
    with pytest.raises(fp.FootprintError, match=r"results depend on the contents"):
        fp.hold(lambda g: k_reads_past_row(g.guard_input(view, "x").t), ME, any_device=True)


def test_allocation_bypassing_the_wrapper_is_reported():
    with pytest.raises(fp.FootprintError, match=r"unguarded device allocation at .*test_footprint_cpu.py:\d+ \(torch factory zeros"):
        _run(k_bypass)
    with fp.guarded(0xFF, ME, any_device=True) as g:
        k_bypass(_x())
        assert len(g.bypassed) == 1
        g.bypassed.clear()


def test_same_bits_tells_nan_payloads_and_signed_zeros_apart():
    a = torch.tensor([0.0, float("nan")])
    assert fp.same_bits(a, a.clone()) and not fp.same_bits(a, torch.tensor([-0.0, float("nan")]))
    assert fp.differences({"a": a, "n": 3}, {"a": a.clone(), "n": 4}) == ["n: 3 vs 4"]


def test_every_entry_point_is_in_the_design_table():
    """DESIGN.md "Memory footprint": every name of _lib.SIGNATURES has a row (held at stated shapes, or excluded with a reason)."""
    import os
    import re

    from topia_xl_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "DESIGN.md"), encoding="utf-8") as fh:
        text = fh.read()
    start = text.index("### Memory footprint")
    section = text[start:text.index("\n## ", start)]
    rows = [ln for ln in section.splitlines() if ln.startswith("|")]
    named = set(re.findall(r"`(primx_\w+)`", "\n".join(rows)))
    missing = sorted(set(_lib.SIGNATURES) - named)
    assert not missing, f"entry points without a row in DESIGN.md's footprint table: {missing}"
    assert not sorted(named - set(_lib.SIGNATURES)), sorted(named - set(_lib.SIGNATURES))
