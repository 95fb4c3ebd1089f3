"""Head dim 80 (up_blocks.2) across the two instantiations of the flash kernel: <80, 2> (512-row workgroups, the loop in
half tiles, a workgroup vote between that body and the one-block-per-wave body) and <80, 1> (256-row workgroups).
Oracle, helper and error bar are those of the D = 80 cases of test_gpu_attention.py.

Which instantiation a launch takes (csrc/attn.hip, launch_flash_auto): <80, 2> when Lq > 256 and
H * ceil(Lq / 512) * B >= the number of CUs (256 on MI355X; the shapes below stay on their side of the rule for any
count from 33 to 256), else <80, 1>."""
import math

import pytest
import torch

import synth
from test_gpu_attention import DEV, _check, _dense_ref

pytestmark = pytest.mark.gpu

H, D = 8, 80
C = H * D
SCALE = 1.0 / math.sqrt(D)


def _qkv(seed, B, Lq, G, M, qgain=1.0):
    g = synth.gen(seed)
    q = (torch.randn(B, Lq, C, generator=g) * qgain).half()
    k = torch.randn(G, M, C, generator=g).half()
    v = torch.randn(G, M, C, generator=g).half()
    return q, k, v


def _run(q, k, v, **kw):
    import fresco_amd.ops as ops
    return ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), H, kw.pop("scale", SCALE), **kw)


# The vote, restated on the CPU for these operands (fold test c |q| max|k| <= 24; no-max-search test: that bound minus the
# first tile's maximum <= 14): q * 0.4 puts every workgroup of the <80, 2> launches on the half-tile body (bound <= 9),
# q * 0.85 splits them (43 to 163 of the 256 workgroups fall back over the shapes below), and with plain N(0,1) q, k
# (bound up to 22.5, the first tile's maximum about 4) every workgroup falls back.
@pytest.mark.parametrize("qgain", [0.4, 0.85, 1.0])
@pytest.mark.parametrize("B,Lq,M", [
    (16, 1024, 1100),   # <80, 2>: the up_blocks.2 cross-frame shape (M not a multiple of 64)
    (2, 1024, 1100),    # <80, 1>: 32 workgroups of 512 rows would leave the chip idle
    (16, 700, 1100),    # <80, 2>, Lq not a multiple of 512 (nor of 256: the second workgroup's last quarter is empty)
    (16, 1000, 333),    # <80, 2>, Lq not a multiple of 512, the last wave partly filled
    (16, 1024, 40),     # one key tile, padded: the half-tile body needs two, every workgroup falls back
    (16, 1024, 100),    # two key tiles, the second padded
    (16, 1024, 128),    # two full key tiles
    (16, 1024, 150),    # three key tiles (nT < 4: the ring never refills)
    (16, 1024, 256),    # four full tiles
    (16, 1024, 321),    # six tiles: one trip of the full-ring loop
])
def test_attention_d80_shapes(B, Lq, M, qgain):
    q, k, v = _qkv(B * 100000 + Lq * 10 + M, B, Lq, B, M, qgain)
    out = _run(q, k, v)
    assert bool(torch.isfinite(out).all())
    _check(out, _dense_ref(q.float(), k.float(), v.float(), H, SCALE, list(range(B))),
           what="D=80 B=%d Lq=%d M=%d qgain=%g" % (B, Lq, M, qgain))


@pytest.mark.parametrize("qgain", [0.4, 0.85])
def test_attention_d80_grouped_rows(qgain):
    """Cross-frame grouping at the <80, 2> shape: 2 groups of 8 frames, keys gathered through a row table."""
    from oracle import fresco_oracle as O
    g = synth.gen(8080)
    chunk, N, HW = 2, 8, 1024
    B = chunk * N
    q = (torch.randn(B, HW, C, generator=g) * qgain).half()
    k = torch.randn(B, HW, C, generator=g).half()
    v = torch.randn(B, HW, C, generator=g).half()
    mask = torch.rand(N, HW, generator=g) < 0.1
    mask[0] = True
    rows = mask.reshape(-1).nonzero().squeeze(1).to(torch.int32)
    out = _run(q, k, v, kv_rows=rows.to(DEV), n_groups=chunk, M=int(rows.numel()), group_rows=N * HW)
    kc = O.compact_cross_frame(k.float(), mask, N, chunk)
    vc = O.compact_cross_frame(v.float(), mask, N, chunk)
    _check(out, _dense_ref(q.float(), kc, vc, H, SCALE, [b // N for b in range(B)]), what="grouped D=80 qgain=%g" % qgain)


@pytest.mark.parametrize("B", [16, 2])
def test_attention_d80_diag_bias(B):
    """The spatial-guided form (scale 0.2 / sqrt(D), diagonal bias): in <80, 2> every workgroup takes the fallback."""
    q, k, v = _qkv(81 + B, B, 1024, B, 1024)
    out = _run(q, k, v, scale=0.2 * SCALE, diag_bias=1.5)
    ref = _dense_ref(q.float(), k.float(), v.float(), H, 0.2 * SCALE, list(range(B)), diag_bias=1.5)
    _check(out, ref, what="diag bias D=80 B=%d" % B)


@pytest.mark.parametrize("qgain", [0.4, 0.85])
@pytest.mark.parametrize("Lq,M", [(1024, 1100), (700, 150)])
def test_attention_d80_both_instantiations_give_equal_bits(Lq, M, qgain):
    """The same (b, h) problems through <80, 2> (16 batch rows in one launch) and <80, 1> (two at a time: below the CU
    threshold).  Key order and k-step order per output element are the same in both bodies, and the fallback of <80, 2> IS
    the <80, 1> body on the same 32-row blocks: equal bits, on the common path (qgain 0.4: every wave folded, no max
    search) and on split votes (qgain 0.85)."""
    B = 16
    q, k, v = _qkv(4242 + Lq + M, B, Lq, B, M, qgain)
    big = _run(q, k, v).cpu()
    for b0 in range(0, B, 2):
        small = _run(q[b0:b0 + 2], k[b0:b0 + 2], v[b0:b0 + 2]).cpu()
        assert torch.equal(big[b0:b0 + 2].view(torch.int16), small.view(torch.int16)), \
            "batch rows %d..%d differ: max |d| %.3e" % (b0, b0 + 1, float((big[b0:b0 + 2].float() - small.float()).abs().max()))
