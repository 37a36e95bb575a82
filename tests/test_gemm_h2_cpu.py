"""The arithmetic of the two-piece fp16 split GEMM (csrc/gemm_split3.hip, SCH = 1) in
torch on the CPU: the piece identities its accuracy rests on, and the three-product
dot product against fp64 beside a sequential fp32 chain.

S = 2^11.  a = a0 + a1 / S with a0 = fp16(a), a1 = fp16(S (a - a0)); the weight row n
is scaled by the power of two r_n that brings its largest magnitude into [1, 2) and
kept as Wm = fp16(S r_n w), Wr = fp16(S r_n w - Wm), W0 = fp16(r_n w); per 16-deep
step acc += a0 Wr; acc += a1 W0; acc += a0 Wm in one fp32 accumulator, and the result
is acc / (S r_n)."""
import math

import pytest
import torch

S = 2048.0


def split_a(a):
    a0 = a.half()
    a1 = ((a - a0.float()) * S).half()
    return a0, a1


def row_exp(w):
    """e with r_n = 2^-e (the kernel's rule: 0 for an all-zero row, held to [-126, 127])."""
    m = w.abs().amax(dim=1).double()
    e = torch.where(m > 0, torch.floor(torch.log2(m.clamp_min(1e-300))), torch.zeros_like(m))
    # log2 of an fp32 value in fp64 is exact enough except at powers of two's neighbours
    e = torch.where((m > 0) & (torch.ldexp(torch.ones_like(m), e.int()) > m), e - 1, e)
    e = torch.where((m > 0) & (torch.ldexp(torch.ones_like(m), (e + 1).int()) <= m), e + 1, e)
    return e.clamp(-126, 127).int()


def split_w(w):
    """(Wm, Wr, W0, scale): the three fp16 images and 1 / (S r_n), from fp64 (S r w is an
    exact scaling, so one rounding to fp16 is the fp32 kernel's rounding)."""
    e = row_exp(w)
    x = torch.ldexp(w.double(), (11 - e).view(-1, 1).expand_as(w))
    wm = x.half()
    wr = (x - wm.double()).half()
    w0 = torch.ldexp(w.double(), (-e).view(-1, 1).expand_as(w)).half()
    return wm, wr, w0, torch.ldexp(torch.ones(len(e), dtype=torch.float64), e - 11).float()


def h2_matmul(a, w):
    """The kernel's sum: one fp32 accumulator, three products per 16-deep step."""
    a0, a1 = (t.float() for t in split_a(a))
    wm, wr, w0, sc = split_w(w)
    wm, wr, w0 = wm.float(), wr.float(), w0.float()
    acc = torch.zeros(a.shape[0], w.shape[0])
    for k in range(0, a.shape[1], 16):
        s = slice(k, k + 16)
        acc = acc + a0[:, s] @ wr[:, s].t()
        acc = acc + a1[:, s] @ w0[:, s].t()
        acc = acc + a0[:, s] @ wm[:, s].t()
    return acc * sc


def chain_matmul(a, w):
    """A sequential fp32 chain over k (one rounding per product, one per add)."""
    acc = torch.zeros(a.shape[0], w.shape[0])
    for k in range(a.shape[1]):
        acc = acc + a[:, k:k + 1] * w[:, k].view(1, -1)
    return acc


def test_activation_pieces_carry_22_bits():
    g = torch.Generator().manual_seed(1)
    mag = torch.exp2(torch.empty(200000).uniform_(-10, math.log2(65504.0), generator=g))
    a = mag * torch.where(torch.rand(200000, generator=g) < .5, -1.0, 1.0)
    a = torch.cat([a, torch.tensor([2.0 ** -10, -2.0 ** -10, 65504.0, -65504.0, 1.0, 0.0,
                                    65503.99, 2049.0, 2.0 ** -10 * (1 + 2.0 ** -23)])])
    a0, a1 = split_a(a)
    assert torch.isfinite(a0.float()).all() and torch.isfinite(a1.float()).all()
    err = (a.double() - a0.double() - a1.double() / S).abs()
    assert bool((err <= 2.0 ** -22 * a.double().abs()).all()), float((err / a.abs()).max())


def test_weight_pieces_carry_22_bits_at_any_magnitude():
    """Rows over fp32's normal range, fp32-subnormal entries, an all-zero row, a row whose
    maximum is a power of two: |S r w - Wm - Wr| <= 2^-22 |S r w| wherever Wr is an fp16
    normal, else 2^-25 absolute (fp16's subnormal spacing: the 2^-36 floor against the
    row's largest magnitude), and W0 within 2^-11."""
    g = torch.Generator().manual_seed(2)
    rows = []
    for ex in (-123, -100, -60, -15, -1, 0, 1, 12, 60, 126):
        rows.append(torch.randn(256, generator=g) * 2.0 ** ex / 4)
    rows.append(torch.zeros(256))
    p2 = torch.randn(256, generator=g).clamp(-.9, .9)
    p2[17] = -1.0
    rows.append(p2 * 2.0 ** -7)
    sub = torch.randn(256, generator=g) * 2.0 ** -130   # fp32-subnormal entries
    sub[3] = 2.0 ** -120
    rows.append(sub)
    w = torch.stack(rows)
    wm, wr, w0, sc = split_w(w)
    e = row_exp(w)
    assert e[10] == 0 and e[11] == -7
    for t in (wm, wr, w0):
        assert torch.isfinite(t.float()).all()
    x = torch.ldexp(w.double(), (11 - e).view(-1, 1).expand_as(w))
    top = x.abs().amax(dim=1)
    assert bool(((top >= 2048) & (top < 4096))[[i for i in range(len(rows)) if i != 10]].all())
    err = (x - wm.double() - wr.double()).abs()
    assert bool((err <= torch.maximum(2.0 ** -22 * x.abs(), torch.tensor(2.0 ** -25,
                                                                       dtype=torch.float64))).all())
    e0 = (x / S - w0.double()).abs()
    assert bool((e0 <= torch.maximum(2.0 ** -11 * (x / S).abs(),
                                     torch.tensor(2.0 ** -25, dtype=torch.float64))).all())
    assert bool((sc.double() == torch.ldexp(torch.ones(len(e), dtype=torch.float64), e - 11)).all())


# mean error of the three-product sum over the sequential fp32 chain's, both against
# fp64 relative to max|y|, measured with this file's emulation (M = 96, N = 64, inputs as
# tests/test_gemm_split3_gpu.py's _case):
#   K = 128: 2.45e-8 / 2.76e-8 = 0.89    K = 256: 2.80e-8 / 3.48e-8 = 0.80
#   K = 1024: 5.01e-8 / 7.45e-8 = 0.67
# (the 16-deep partial sums shorten the chain; at small K the pieces' 2^-22
# representation error shows beside fp32's 2^-24).  The bound: the largest measured
# ratio with a 40 % allowance for another host's summation order inside a 16-deep step.
FACTOR = 1.25


@pytest.mark.parametrize("K", [128, 256, 1024])
def test_three_product_dot_against_fp64(K):
    g = torch.Generator().manual_seed(K)
    a = torch.randn(96, K, generator=g).relu_()
    w = torch.randn(64, K, generator=g) / K ** .5
    ref = a.double() @ w.double().t()
    s = float(ref.abs().max())
    h2 = float((h2_matmul(a, w).double() - ref).abs().mean()) / s
    ch = float((chain_matmul(a, w).double() - ref).abs().mean()) / s
    print("K=%d h2 mean %.3g chain mean %.3g ratio %.2f" % (K, h2, ch, h2 / ch))
    assert h2 <= FACTOR * ch, (h2, ch)
    mx = float((h2_matmul(a, w).double() - ref).abs().max()) / s
    assert mx <= 2e-5
