"""The row-per-workgroup and element-wise HIP kernels (norm.hip, quant.hip's quant_rowwise /
silu_mul_quant / quant_rowwise_int8, activation.hip) against the fp64 oracles and derived bounds
of tests/row_oracle.py, at the smallest widths that reach every (threads, VPT) instantiation of
the launchers, on input families where a dropped vector, a wrong divisor, a missing eps, a
truncating store or a lane left out of amax is an error far above the bound.

Besides the bounds: bit-exact invariances (in-place residual == residual_out, inputs untouched,
two calls identical, row order, independence of the other rows), guard regions around every
output, and the shapes the launchers must reject without writing.

Each test prints the largest err / bound per kernel and family as ``ROW-RATIO gpu <kernel>
<family> <ratio>`` and the largest share of codes that differ from the fp64 codes as ``ROW-SHARE``
(run with -s to see them; docs/kernels.md quotes them).

Run on an MI355X: ``python -m pytest tests/test_row_kernels_gpu.py -m gpu``.
"""
import pytest
import torch

import row_oracle as ro
from distributed_llm_inference import ops

pytestmark = pytest.mark.gpu
BF = ro.BF
G = 4096                # guard elements on each side
SENT = -12345.0
SENT8 = 0x5A


def _check_cases(gpu, name, cases):
    worst, share, fails = {}, 0.0, []
    for c in cases:
        v = ro.evaluate(c, ro.run_ops(c, gpu))
        key = (c.kernel, c.family)
        worst[key] = max(worst.get(key, 0.0), v.ratio)
        share = max(share, v.share)
        fails += [f"{c.ident()}: {p}" for p in v.problems]
    for (k, fam), r in sorted(worst.items()):
        print(f"ROW-RATIO gpu {k} {fam} {r:.4f}")
    print(f"ROW-SHARE gpu {name} {share:.2e}")
    assert not fails, "\n".join(fails[:20])


# ------------------------------------------------------------------------------------ bounds
@pytest.mark.parametrize("kind", ["rms", "ln"])
@pytest.mark.parametrize("H", ro.NORM_WIDTHS)
def test_norm(gpu, kind, H):
    _check_cases(gpu, f"{kind}-{H}", [c for c in ro.norm_cases(kind) if c.H == H])


@pytest.mark.parametrize("kind", ["rms", "quant"])
def test_splitk_partials_input(gpu, kind):
    """x given as S = 1 / 8 fp32 / bf16 partials: the fp32 sum in split order, rounded once."""
    _check_cases(gpu, f"{kind}-parts", ro.parts_cases(kind))


@pytest.mark.parametrize("H", ro.QUANT_WIDTHS)
def test_quant_rowwise(gpu, H):
    _check_cases(gpu, f"quant-{H}", [c for c in ro.quant_cases() if c.H == H])


@pytest.mark.parametrize("H", ro.QUANT_WIDTHS)
def test_silu_mul_quant(gpu, H):
    _check_cases(gpu, f"silu_mul_quant-{H}", [c for c in ro.silu_quant_cases() if c.H == H])


@pytest.mark.parametrize("H", ro.QUANT_WIDTHS)
def test_quant_rowwise_int8(gpu, H):
    _check_cases(gpu, f"int8-{H}", [c for c in ro.int8_cases() if c.H == H])


@pytest.mark.parametrize("kernel", ["silu_mul", "silu_il", "gelu", "add"])
def test_elementwise(gpu, kernel):
    """Includes one 70 x 65536 case per kernel: the grid-stride loop's second trip."""
    _check_cases(gpu, kernel, [c for c in ro.elementwise_cases() if c.kernel == kernel])


# ------------------------------------------------------------------------------- invariances
INVARIANT_CASES = [
    ro.Case("rms", 2056, "gauss", residual=True),
    ro.Case("rms", 10248, "spike", residual=True, eps=1e-6),
    ro.Case("rms", 520, "gauss", parts=(8, "f32"), residual=True),
    ro.Case("ln", 5120, "offset", residual=True, wkind="gauss"),
    ro.Case("ln", 16384, "heavy"),
    ro.Case("quant", 8200, "gauss", norm=True, residual=True),
    ro.Case("quant", 65544, "heavy"),
    ro.Case("quant", 10248, "gauss", parts=(8, "bf16"), norm=True, residual=True),
    ro.Case("silu_mul_quant", 4104, "heavy"),
    ro.Case("int8", 32776, "gauss", mask=True),
    ro.Case("silu_mul", 520, "heavy"),
    ro.Case("silu_il", 384, "gauss"),
    ro.Case("gelu", 8000, "gauss"),
    ro.Case("add", 520, "big"),
]


def _same(a: dict, b: dict, rows=None):
    for n in a:
        x, y = a[n], b[n]
        if rows is not None:
            x, y = x.reshape(x.shape[0], -1)[rows], y.reshape(y.shape[0], -1)[rows]
        x, y = x.contiguous(), y.contiguous()
        if not torch.equal(x.view(torch.uint8), y.view(torch.uint8)):
            return n
    return None


def _rowwise(inp: dict, fn) -> dict:
    """``fn`` applied to every per-row tensor of the inputs (partials: along dim 1)."""
    out = dict(inp)
    for n in ("x", "res", "gate", "up"):
        if n in inp:
            out[n] = fn(inp[n], 0)
    if "parts" in inp:
        out["parts"] = fn(inp["parts"], 1)
    return out


@pytest.mark.parametrize("c", INVARIANT_CASES, ids=ro.ids(INVARIANT_CASES))
def test_invariances(gpu, c):
    inp = ro.inputs(c)
    dev = {n: (t.to(gpu) if torch.is_tensor(t) else t) for n, t in inp.items()}
    before = {n: t.clone() for n, t in dev.items() if torch.is_tensor(t)}
    out = ro.run_ops(c, gpu, dev)
    torch.cuda.synchronize()
    for n, t in before.items():
        assert torch.equal(t.view(torch.uint8), dev[n].view(torch.uint8)), f"input {n} was modified"
    assert _same(out, ro.run_ops(c, gpu, dev)) is None, "two calls differ"
    # reversed row order
    flip = _rowwise(inp, lambda t, d: t.flip(d).contiguous())
    out_f = ro.run_ops(c, gpu, flip)
    bad = _same(out, {n: t.flip(0) for n, t in out_f.items()})
    assert bad is None, f"{bad}: reversing the rows does not reverse the outputs"
    # every row but one replaced
    keep = 2

    def others(t, d):
        t2 = (-t.float()).roll(1, dims=d).to(t.dtype)
        t2.select(d, keep).copy_(t.select(d, keep))
        return t2.contiguous()
    out_o = ro.run_ops(c, gpu, _rowwise(inp, others))
    bad = _same(out, out_o, rows=keep)
    assert bad is None, f"{bad}: row {keep} depends on the other rows"
    assert _same(out, out_o) is not None, "the other rows were not replaced"
    # in-place residual == out-of-place residual_out
    if c.residual:
        res = dev["res"].clone()
        x = ops.SplitKPartials(dev["parts"]) if c.parts else dev["x"]
        if c.kernel == "rms":
            y, r = ops.rms_norm(x, dev["w"], c.eps, residual=res)
            got = dict(y=y.cpu(), r=r.cpu())
        elif c.kernel == "ln":
            y, r = ops.layer_norm(x, dev["w"], dev["b"], c.eps, residual=res)
            got = dict(y=y.cpu(), r=r.cpu())
        else:
            q, s = ops.quant_rowwise(x, residual=res, norm_w=dev.get("w"), eps=c.eps)
            got = dict(q=q.view(torch.uint8).cpu(), s=s.cpu(), r=res.cpu())
        bad = _same(out, got)
        assert bad is None, f"{bad}: in-place residual differs from residual_out"


# ------------------------------------------------------------------------------------ guards
def _guarded(shape, dtype, dev):
    n = 1
    for s in shape:
        n *= s
    if dtype in (torch.uint8, torch.int8):
        buf = torch.full((G + n + G,), SENT8, dtype=dtype, device=dev)
    else:
        buf = torch.full((G + n + G,), SENT, dtype=dtype, device=dev)
    return buf, buf[G:G + n].view(*shape)


def _is_sent(t):
    """Element-wise: still the sentinel of the tensor's type."""
    s = SENT8 if t.dtype in (torch.uint8, torch.int8) else SENT
    return t == torch.tensor(s, dtype=t.dtype, device=t.device)


def _guards_intact(buf, n, what):
    assert bool(_is_sent(buf[:G]).all()), f"{what}: write before the output"
    assert bool(_is_sent(buf[G + n:]).all()), f"{what}: write after the output"


@pytest.mark.parametrize("H", [2056, 10248])
def test_norm_guards(gpu, H):
    rows = 5
    x = ro.family("gauss", H, ro.norm_arm(H)[:2], "gx", rows).to(gpu)
    res = ro.family("gauss", H, ro.norm_arm(H)[:2], "gr", rows).to(gpu)
    w = torch.ones(H, dtype=BF, device=gpu)
    b = torch.zeros(H, dtype=BF, device=gpu)
    for name in ("rms", "ln"):
        obuf, out = _guarded((rows, H), BF, gpu)
        rbuf, rout = _guarded((rows, H), BF, gpu)
        if name == "rms":
            ops.rms_norm(x, w, 1e-5, residual=res, out=out, residual_out=rout)
            want, _ = ops.rms_norm(x, w, 1e-5, residual=res.clone())
        else:
            ops.layer_norm(x, w, b, 1e-5, residual=res, out=out, residual_out=rout)
            want, _ = ops.layer_norm(x, w, b, 1e-5, residual=res.clone())
        torch.cuda.synchronize()
        _guards_intact(obuf, rows * H, f"{name} out")
        _guards_intact(rbuf, rows * H, f"{name} residual_out")
        assert torch.equal(out, want) and torch.equal(rout.cpu(), ro.bf16_add(x.cpu(), res.cpu()))
    for fn, name in ((lambda o: ops.gelu_bias(x, b, out=o), "gelu"),
                     (lambda o: ops.add(x, res, out=o), "add")):
        obuf, out = _guarded((rows, H), BF, gpu)
        fn(out)
        torch.cuda.synchronize()
        _guards_intact(obuf, rows * H, name)
    obuf, out = _guarded((rows, H), BF, gpu)
    ops.silu_mul(torch.cat([x, res], dim=1).contiguous(), out=out)
    torch.cuda.synchronize()
    _guards_intact(obuf, rows * H, "silu_mul")


@pytest.mark.parametrize("H", [2056, 10248, 32776, 65544])
def test_quant_guards(gpu, H):
    rows = 5
    C = ops.native()
    arm = ro.quant_arm(H)[:2]
    x = ro.family("gauss", H, arm, "gx", rows).to(gpu)
    res = ro.family("gauss", H, arm, "gr", rows).to(gpu)
    w = torch.ones(H, dtype=BF, device=gpu)
    xx = torch.cat([x, res], dim=1).contiguous()
    mask = torch.zeros(H, dtype=torch.uint8, device=gpu)
    mask[::41] = 1
    runs = (
        ("quant", torch.uint8, lambda q, s, r: C.quant_rowwise(q, s, x, None, None, 0.0, None)),
        ("quant+norm+res", torch.uint8,
         lambda q, s, r: C.quant_rowwise(q, s, x, res, w, 1e-5, r)),
        ("silu_mul_quant", torch.uint8, lambda q, s, r: C.silu_mul_quant(q, s, xx)),
        ("int8", torch.int8, lambda q, s, r: C.quant_rowwise_int8(q, s, x, mask)),
    )
    for name, qdt, fn in runs:
        qbuf, q = _guarded((rows, H), qdt, gpu)
        sbuf, s = _guarded((rows,), torch.float32, gpu)
        rbuf, r = _guarded((rows, H), BF, gpu)
        fn(q, s, r)
        torch.cuda.synchronize()
        _guards_intact(qbuf, rows * H, f"{name} q")
        _guards_intact(sbuf, rows, f"{name} scale")
        _guards_intact(rbuf, rows * H, f"{name} residual_out")
        assert not bool(_is_sent(s).any()), f"{name}: a scale was not written"
        if "res" in name:
            assert torch.equal(r.cpu(), ro.bf16_add(x.cpu(), res.cpu()))
        else:
            assert bool(_is_sent(r).all()), f"{name}: wrote residual_out"


# -------------------------------------------------------------------------------- rejections
def _rejects(gpu, what, fn, outs):
    """``fn`` must raise and leave every output at its sentinel."""
    with pytest.raises(RuntimeError):
        fn()
    torch.cuda.synchronize()
    for o in outs:
        assert bool(_is_sent(o).all()), f"{what}: the rejected call wrote its output"


def _outs(gpu, rows, H, qdt=torch.uint8):
    return (torch.full((rows, H), SENT, dtype=BF, device=gpu),
            torch.full((rows, H), SENT8, dtype=qdt, device=gpu),
            torch.full((rows,), SENT, dtype=torch.float32, device=gpu))


@pytest.mark.parametrize("H,which", [(12, "all"), (16392, "norm"), (131080, "quant")])
def test_rejected_widths(gpu, H, which):
    """A width that is no multiple of 8, the first norm width past VPT 8 x 256 threads and the
    first quantiser width past VPT 16 x 1024 threads."""
    rows = 2
    C = ops.native()
    x = torch.ones(rows, H, dtype=BF, device=gpu)
    w = torch.ones(H, dtype=BF, device=gpu)
    y, q, s = _outs(gpu, rows, H)
    q8 = torch.full((rows, H), SENT8, dtype=torch.int8, device=gpu)
    r = torch.full((rows, H), SENT, dtype=BF, device=gpu)
    if which in ("all", "norm"):
        _rejects(gpu, "rms_norm", lambda: C.rms_norm(y, x, x.clone(), w, 1e-5, r), (y, r))
        _rejects(gpu, "layer_norm", lambda: C.layer_norm(y, x, x.clone(), w, w, 1e-5, r), (y, r))
    if which in ("all", "quant"):
        _rejects(gpu, "quant_rowwise",
                 lambda: C.quant_rowwise(q, s, x, x.clone(), w, 1e-5, r), (q, s, r))
        _rejects(gpu, "quant_rowwise_int8", lambda: C.quant_rowwise_int8(q8, s, x, None), (q8, s))
        xx = torch.ones(rows, 2 * H, dtype=BF, device=gpu)
        _rejects(gpu, "silu_mul_quant", lambda: C.silu_mul_quant(q, s, xx), (q, s))
    if which == "all":
        xx = torch.ones(rows, 2 * H, dtype=BF, device=gpu)
        _rejects(gpu, "silu_mul", lambda: C.silu_mul(y, xx), (y,))
        _rejects(gpu, "gelu_bias", lambda: C.gelu_bias(y, x, w), (y,))
        y1 = torch.full((H,), SENT, dtype=BF, device=gpu)
        _rejects(gpu, "add", lambda: C.add(y1, x[0], x[1]), (y1,))


@pytest.mark.parametrize("pdt", [torch.float32, BF])
def test_rejected_nine_partials(gpu, pdt):
    rows, H = 2, 520
    C = ops.native()
    parts = torch.ones(9, rows, H, dtype=pdt, device=gpu)
    w = torch.ones(H, dtype=BF, device=gpu)
    y, q, s = _outs(gpu, rows, H)
    _rejects(gpu, "rms_norm_splitk", lambda: C.rms_norm_splitk(y, parts, None, w, 1e-5, None), (y,))
    _rejects(gpu, "quant_rowwise", lambda: C.quant_rowwise(q, s, parts, None, None, 0.0, None),
             (q, s))


def test_rejected_non_contiguous_x(gpu):
    rows, H = 3, 520
    C = ops.native()
    x = torch.ones(rows, 2 * H, dtype=BF, device=gpu)[:, :H]
    assert not x.is_contiguous()
    w = torch.ones(H, dtype=BF, device=gpu)
    y, q, s = _outs(gpu, rows, H)
    q8 = torch.full((rows, H), SENT8, dtype=torch.int8, device=gpu)
    _rejects(gpu, "rms_norm", lambda: C.rms_norm(y, x, None, w, 1e-5, None), (y,))
    _rejects(gpu, "layer_norm", lambda: C.layer_norm(y, x, None, w, w, 1e-5, None), (y,))
    _rejects(gpu, "gelu_bias", lambda: C.gelu_bias(y, x, None), (y,))
    _rejects(gpu, "add", lambda: C.add(y, x, x), (y,))
    _rejects(gpu, "quant_rowwise", lambda: C.quant_rowwise(q, s, x, None, None, 0.0, None), (q, s))
    _rejects(gpu, "quant_rowwise_int8", lambda: C.quant_rowwise_int8(q8, s, x, None), (q8, s))
    y2 = torch.full((rows, H // 2), SENT, dtype=BF, device=gpu)
    q2 = torch.full((rows, H // 2), SENT8, dtype=torch.uint8, device=gpu)
    _rejects(gpu, "silu_mul", lambda: C.silu_mul(y2, x), (y2,))
    _rejects(gpu, "silu_mul_quant", lambda: C.silu_mul_quant(q2, s, x), (q2, s))
