"""The fused MLP kernel K30 (ops/hip/mlp_encode.hip, whose header states the
operation and layout) against plain int64 / fp64 forward passes.
ANOVOS_MLP_BLOCKS forces the grid, so small inputs reach the multi-slab paths
and blocks that own only the partial slab, or nothing (n = 200, 3 blocks).
The weight image is one ring stage per output tile, so every image spans
several stages: 5 at d = 2, 37 at d = 150.

Derived bound, largest |got - ref| / bound seen: see docs/KERNELS.md, K30."""

import pytest
import torch

pytestmark = [pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X"), pytest.mark.gpu]

DEV = "cuda"
NAN = float("nan")


@pytest.fixture(scope="module")
def ext():
    from anovos_amd.ops import backend

    return backend.require_hip()


def _ae(d):
    return (d, 2 * d, max(d // 2, 1), max(d // 2, 1))


def _forward(z, layers, exact=False):
    """y [n3, n] of z [d, n] in fp64, or in int64 with the conditions that make
    the kernel exact asserted on the way: every sum |w| |a| + |b| below 2^24
    and every hidden activation below 2^16 (hi + lo holds it)."""
    a = z.long() if exact else z.double()
    for i, (W, b) in enumerate(layers):
        W, b = (W.long(), b.long()) if exact else (W.double(), b.double())
        if exact:
            assert int((W.abs() @ a.abs() + b.abs()[:, None]).max()) < 2 ** 24
        a = W @ a + b[:, None]
        if i < 2:
            a = a.clamp(min=0)
            assert not exact or int(a.max()) < 2 ** 16
    return a


def _run(ext, x, shift, scale, layers, outs=None):
    xd = x.to(DEV)
    got = ext.mlp_encode_bf16x2([xd[i] for i in range(xd.shape[0])], shift.to(DEV), scale.to(DEV),
                                *[t.to(DEV) for Wb in layers for t in Wb], outs)
    assert len(got) == layers[2][0].shape[0]
    assert all(t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (x.shape[1],) for t in got)
    return torch.stack([t.cpu() for t in got])


def _int_case(shape, n, g):
    """x integers in [-2, 2] with 5 % NaN, one all-NaN row and one all-NaN
    column; integer shifts; weights in {-1, 0, 1}; biases in [-3, 3]"""
    d = shape[0]
    x = torch.randint(-2, 3, (d, n), generator=g).float()
    x[torch.rand(d, n, generator=g) < 0.05] = NAN
    if n > 1:
        x[:, n // 2] = NAN
    if d > 1:
        x[d // 2] = NAN
    shift = torch.randint(-2, 3, (d,), generator=g).float()
    layers = [(torch.randint(-1, 2, (o, i), generator=g).float(), torch.randint(-3, 4, (o,), generator=g).float())
              for i, o in zip(shape[:3], shape[1:])]
    return x, shift, layers


SHAPES = [_ae(d) for d in (2, 8, 31, 32, 33, 64, 96, 150, 160)] + [
    # free widths at tile edges, d = 40 (KS = 2: n1 <= 128, n2, n3 <= 64)
    (40, 1, 1, 1), (40, 15, 16, 15), (40, 16, 17, 16), (40, 17, 33, 17), (40, 31, 64, 1), (40, 32, 32, 15),
    (40, 33, 31, 17), (40, 128, 64, 64)]


@pytest.mark.parametrize("blocks", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_exact_small_integers(ext, monkeypatch, shape, blocks):
    monkeypatch.setenv("ANOVOS_MLP_BLOCKS", str(blocks))
    g = torch.Generator().manual_seed(3000 + sum(shape))
    for n in (1, 15, 16, 17, 63, 64, 65, 129, 200, 516):
        x, shift, layers = _int_case(shape, n, g)
        z = torch.where(torch.isnan(x), torch.zeros_like(x), x - shift[:, None])
        ref = _forward(z, layers, exact=True)
        got = _run(ext, x, shift, torch.ones(shape[0]), layers)
        assert torch.equal(got.long(), ref) and torch.equal(got, got.round()), f"shape={shape} n={n} blocks={blocks}"


def _placed(o, i, g, values=None):
    """[o, i] with one entry per row (1, or values[row]) on a partial
    permutation: distinct columns while they last"""
    W = torch.zeros(o, i)
    col = torch.cat([torch.randperm(i, generator=g) for _ in range((o + i - 1) // i)])[:o]
    W[torch.arange(o), col] = torch.ones(o) if values is None else values
    return W


@pytest.mark.parametrize("plane", ["z", "W1", "W2", "W3"])
def test_exact_lo_planes(ext, monkeypatch, plane):
    """odd 16-bit positive integers, which plain bf16 would miss, in x (they
    pass through all three layers: the lo planes of z, a1 and a2) or in one
    layer's weights against inputs of 1; four draws of the placement per shape"""
    monkeypatch.setenv("ANOVOS_MLP_BLOCKS", "3")
    g = torch.Generator().manual_seed(3001)
    odd = lambda *s: (torch.randint(2 ** 7, 2 ** 15, s, generator=g) * 2 + 1).float()
    for shape in [_ae(150), _ae(150), (40, 128, 64, 64), (33, 17, 33, 17)]:
        d, n = shape[0], 129
        x = odd(d, n) if plane == "z" else torch.ones(d, n)
        layers = [(_placed(o, i, g, odd(o) if plane == f"W{l + 1}" else None), torch.zeros(o))
                  for l, (i, o) in enumerate(zip(shape[:3], shape[1:]))]
        got = _run(ext, x, torch.zeros(d), torch.ones(d), layers)
        assert torch.equal(got.long(), _forward(x, layers, exact=True)), f"{plane} shape={shape}"


@pytest.mark.parametrize("d", [16, 32, 150])
def test_derived_bound(ext, monkeypatch, d):
    """Real x with |mean| up to 1e4 sigma, 5 % NaN, the autoencoder's default
    initialisation; reference fp64 on the same f32 z. Per layer, with a^ the
    computed input (|a^| <= |a_ref| + e) and ReLU 1-Lipschitz:
      e_l = gamma_l (|W_l| |a^_{l-1}| + |b_l|) + |W_l| e_{l-1}
      gamma_l = 3 * 2^-18 + (3 * kpad_l + 1) * 2^-24
    - 2^-18 for each operand's split residual and for the dropped lo.lo term,
    and the fp32 sum of 3 * kpad_l products and the bias, kpad_l the layer's
    inputs padded to 32."""
    from anovos_amd.data_transformer.transformers_advanced import _AE

    monkeypatch.setenv("ANOVOS_MLP_BLOCKS", "3")
    torch.manual_seed(3010 + d)
    g = torch.Generator().manual_seed(3010 + d)
    enc = _AE(d, max(1, d // 2)).encoder
    layers = [(enc[i].weight.detach(), enc[i].bias.detach()) for i in (0, 2, 4)]
    n = 333
    sd = 0.5 + 2 * torch.rand(d, generator=g)
    shift = 10 * torch.randn(d, generator=g)
    shift[::5] *= 1000
    x = torch.randn(d, n, generator=g) * sd[:, None] + shift[:, None]
    x[torch.rand(d, n, generator=g) < 0.05] = NAN
    scale = 1 / sd
    z = torch.where(torch.isnan(x), torch.zeros_like(x), (x - shift[:, None]) * scale[:, None])
    ref = _forward(z, layers)
    a, e = z.double().abs(), torch.zeros(d, n, dtype=torch.float64)
    for i, (W, b) in enumerate(layers):
        gamma = 3 * 2.0 ** -18 + (3 * ((W.shape[1] + 31) // 32 * 32) + 1) * 2.0 ** -24
        Wa = W.double().abs()
        e = gamma * (Wa @ (a + e) + b.double().abs()[:, None]) + Wa @ e
        a = _forward(z, layers[: i + 1]) if i < 2 else None  # the reference activation, >= 0
    got = _run(ext, x, shift, scale, layers).double()
    assert torch.equal(got, _run(ext, x, shift, scale, layers).double()), "the same call returned different bits"
    ratio = (got - ref).abs() / e
    print(f"mlp_encode derived bound d={d}: max |got-ref|/bound = {float(ratio.max()):.4f}")
    assert bool((ratio <= 1).all()), f"d={d}: {int((ratio > 1).sum())} outputs beyond the bound, worst {float(ratio.max())}"


@pytest.mark.parametrize("n", [1, 63, 65, 130])
def test_caller_owned_outs(ext, monkeypatch, n):
    """views buf[c, 4 : 4 + n] of a guard-filled buffer: exact outputs, every
    guard element untouched; a view at element offset 1 is refused"""
    monkeypatch.setenv("ANOVOS_MLP_BLOCKS", "3")
    g = torch.Generator().manual_seed(3020 + n)
    shape, guard = (33, 66, 17, 17), -12345.0
    x, shift, layers = _int_case(shape, n, g)
    z = torch.where(torch.isnan(x), torch.zeros_like(x), x - shift[:, None])
    ref = _forward(z, layers, exact=True)
    buf = torch.full((17, (n + 8 + 3) // 4 * 4), guard, device=DEV)
    got = _run(ext, x, shift, torch.ones(33), layers, [buf[c, 4:4 + n] for c in range(17)])
    host = buf.cpu()
    assert torch.equal(got.long(), ref) and torch.equal(host[:, 4:4 + n], got)
    assert bool((host[:, :4] == guard).all()) and bool((host[:, 4 + n:] == guard).all())
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        _run(ext, x, shift, torch.ones(33), layers, [buf[c, 1:1 + n] for c in range(17)])


def test_argument_checks(ext):
    def call(d=4, widths=(8, 2, 2), n=8, col_dev=DEV, w_dev=DEV, nshift=None, b1=None, w2_in=None):
        cols = [torch.zeros(n, device=col_dev) for _ in range(d)]
        ins = [d, widths[0] if w2_in is None else w2_in, widths[1]]
        params = [t for i, o in zip(ins, widths) for t in (torch.zeros(o, i, device=w_dev), torch.zeros(o, device=w_dev))]
        if b1 is not None:
            params[1] = torch.zeros(b1, device=w_dev)
        vec = torch.ones(d if nshift is None else nshift, device=DEV)
        return ext.mlp_encode_bf16x2(cols, vec, torch.ones(d, device=DEV), *params)

    for match, kw in [
        ("at most 160", dict(d=161, widths=(8, 2, 2))),
        ("layer widths", dict(d=32, widths=(65, 2, 2))),
        ("layer widths", dict(d=32, widths=(64, 33, 2))),
        ("layer widths", dict(d=40, widths=(64, 64, 65))),
        ("W2 must be", dict(w2_in=7)),
        ("length mismatch", dict(b1=7)),
        ("shift has 3 entries, expected 4", dict(nshift=3)),
        ("device columns required", dict(col_dev="cpu")),
        ("on the columns' device", dict(w_dev="cpu")),
    ]:
        with pytest.raises(RuntimeError, match=match):
            call(**kw)
    empty = call(n=0)
    assert len(empty) == 2 and all(t.dtype == torch.float32 and tuple(t.shape) == (0,) for t in empty)
