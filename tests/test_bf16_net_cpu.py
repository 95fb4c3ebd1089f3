"""The bf16 forms of vae_conv, unet_groupnorm and unet_temb and the bf16 UNetResnet, without a GPU:

  1. the C entry points' argument checks with the bf16 flag / dtype: every bad argument tests/test_vae_cpu.py and
     tests/test_unet_resnet_cpu.py try is tried again with it and must get the answer the fp16 form gives (fake pointers:
     every check answers before any HIP call);
  2. the Python surface on the stand-in tree at c = 64 in bf16;
  3. the hipcc listing of csrc/net_bf16.hip, compiled the way tests/test_kernel_resources_vae.py and _unet.py compile theirs:
     exactly the bf16 twins, no spill, no scratch, the fp16 kernels' LDS and register bars, the bf16 MFMA and the LDS-DMA, no
     fp16 MFMA, no atomics.
"""
import os
import re
import shutil
import subprocess

import pytest
import torch

import unet_resnet_bf16_model as B
import unet_resnet_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fresco_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only"]
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
BF16_FLAG = 0x100     # VAE_ELEM_BF16 = UNET_ELEM_BF16
F16, BF16 = 0, 2      # FRESCO_F16, FRESCO_BF16


@pytest.fixture(scope="module")
def lib():
    from fresco_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------------
# 1. argument checks
# ---------------------------------------------------------------------------------------------------------------------
def test_headers_and_binding_name_the_flag():
    from fresco_amd import _lib
    vae = open(os.path.join(ROOT, "include", "fresco_vae.h")).read()
    unet = open(os.path.join(ROOT, "include", "fresco_unet.h")).read()
    assert re.search(r"^#define VAE_ELEM_BF16 0x100$", vae, re.M) and re.search(r"^#define UNET_ELEM_BF16 0x100$", unet, re.M)
    assert _lib.ELEM_BF16 == BF16_FLAG and (_lib.F16, _lib.BF16) == (F16, BF16)
    assert re.search(r"^int unet_temb_dt\(", unet, re.M) and "unet_temb_dt" in _lib.UNET_SIGNATURES
    assert _lib.UNET_SIGNATURES["unet_temb_dt"][1][:8] == _lib.UNET_SIGNATURES["unet_temb"][1][:8]
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "net_bf16.hip" in re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    assert not re.search(r"build/net_bf16\.o[^\n]*EXTRA", mk)   # plain flags: FLAGS above is the whole command line


def test_conv_argument_checks_with_the_bf16_flag(lib):
    p = 4096  # fake, aligned, never touched
    base = dict(x=p, xs=10 * 14 * 128, w=p, ws=0, bias=p, res=0, out=p, n=2, H=10, W=14, cin=128, cout=128, k=3, up2=0, kind=0,
                brows=0, ldo=128, st=0)
    bad = [  # tests/test_vae_cpu.py's list, with the code each gets
        (dict(x=0), EINVAL), (dict(w=0), EINVAL), (dict(out=0), EINVAL), (dict(n=0), EINVAL), (dict(H=0), EINVAL),
        (dict(cout=0), EINVAL), (dict(cin=-32), EINVAL), (dict(kind=3), EINVAL), (dict(ldo=64), EINVAL), (dict(x=p + 8), EINVAL),
        (dict(w=p + 2), EINVAL), (dict(out=p + 4), EINVAL), (dict(bias=p + 4), EINVAL), (dict(res=p + 2), EINVAL),
        (dict(res=p, kind=1), EINVAL), (dict(xs=128), EINVAL), (dict(brows=1), EINVAL), (dict(k=1, up2=1), EINVAL),
        (dict(ws=-8), EINVAL), (dict(ws=12), EINVAL), (dict(kind=2, ldo=256), EINVAL), (dict(k=5), EUNSUPPORTED),
        (dict(k=2), EUNSUPPORTED), (dict(cin=4, xs=10 * 14 * 4), EUNSUPPORTED), (dict(cin=144, xs=10 * 14 * 144), EUNSUPPORTED),
        (dict(up2=1, H=9, xs=4 * 7 * 128), EUNSUPPORTED), (dict(n=65536), EUNSUPPORTED),
        (dict(n=1, H=65536, W=32768, xs=65536 * 32768 * 128), EUNSUPPORTED),
        (dict(n=1, H=(1 << 31) - 1, W=1, k=1, xs=0, cout=1 << 20, ldo=1 << 20), EUNSUPPORTED)]
    for change, code in bad:
        args = dict(base, **change)
        assert lib.vae_conv(*args.values()) == code, change
        args["kind"] |= BF16_FLAG
        assert lib.vae_conv(*args.values()) == code, ("bf16", change)
    # the flag on an output kind that does not exist, and bits that are no flag
    assert lib.vae_conv(*dict(base, kind=3 | BF16_FLAG).values()) == EINVAL
    for unknown in (0x200, 0x80, 0x1000 | BF16_FLAG, 4, 1 << 30):
        assert lib.vae_conv(*dict(base, kind=unknown).values()) == EINVAL, hex(unknown)


def test_groupnorm_argument_checks_with_the_bf16_flag(lib):
    p = 4096
    n, P, C = 2, 4096, 320
    need = lib.unet_groupnorm_workspace_bytes(n, P, C)

    def call(flags, x=p, addend=None, gamma=p, beta=p, y=p, ws=p, wsb=need, n=n, P=P, C=C, eps=1e-5):
        return lib.unet_groupnorm(x, addend, gamma, beta, y, ws, wsb, n, P, C, eps, flags, None)

    bad = [(dict(C=c), EUNSUPPORTED) for c in (96, 2624, 32, 2500)] + [(dict(wsb=need - 1), EWORKSPACE), (dict(wsb=0), EWORKSPACE)]
    bad += [({null: None}, EINVAL) for null in ("x", "gamma", "beta", "y", "ws")]
    bad += [(dict(n=0), EINVAL), (dict(P=0), EINVAL), (dict(C=-64), EINVAL), (dict(eps=-1.0), EINVAL), (dict(eps=float("nan")), EINVAL),
            (dict(x=p + 8), EINVAL), (dict(addend=p + 4), EINVAL), (dict(y=p + 2), EINVAL), (dict(n=65536, wsb=1 << 40), EUNSUPPORTED),
            (dict(n=1024, P=1 << 21, wsb=1 << 40), EUNSUPPORTED), (dict(P=64, wsb=0), EWORKSPACE)]
    for change, code in bad:
        for flags in (1, 0, 1 | BF16_FLAG, BF16_FLAG):
            assert call(flags, **change) == code, (change, hex(flags))
    # the word is flags now: bit 0 and the element bit; any other bit is refused (with otherwise valid arguments)
    for unknown in (2, 0x200, 0x80 | BF16_FLAG, 1 << 30, -2):
        assert call(unknown) == EINVAL, unknown
    # the workspace and the form do not depend on the element type: both are 2 bytes wide (nothing to pass a flag to)
    assert lib.unet_groupnorm_lds_form(n, 64, C) == 1 and lib.unet_groupnorm_lds_form(n, P, C) == 0


def test_temb_argument_checks_with_a_dtype(lib):
    p = 4096

    def call(dtype, temb=p, w=p, bias=p, cbias=p, out=p, n=16, K=1280, cout=320):
        return lib.unet_temb_dt(temb, w, bias, cbias, out, n, K, cout, dtype, None)

    bad = [(dict(n=65), EUNSUPPORTED), (dict(K=1284), EUNSUPPORTED)]
    bad += [({null: None}, EINVAL) for null in ("temb", "w", "bias", "cbias", "out")]
    bad += [(dict(n=0), EINVAL), (dict(K=0), EINVAL), (dict(cout=0), EINVAL), (dict(temb=p + 8), EINVAL), (dict(w=p + 2), EINVAL),
            (dict(out=p + 2), EINVAL)]
    for change, code in bad:
        assert call(F16, **change) == code and call(BF16, **change) == code, change
    for unknown in (1, 3, -1, BF16_FLAG):     # fp32 and codes that are none
        assert call(unknown) == EINVAL, unknown


# ---------------------------------------------------------------------------------------------------------------------
# 2. the Python surface
# ---------------------------------------------------------------------------------------------------------------------
def _tree():
    return B.build_tree(torch.bfloat16, c=64)


def test_bf16_tree_is_patched_and_packed():
    from fresco_amd import UNetResnet, patch_unet_resnets, unpatch_unet_resnets
    tree = _tree()
    blocks = [m for m in tree.modules() if isinstance(m, M.Resnet)]
    assert patch_unet_resnets(tree, dtype=torch.bfloat16) == 2
    for b in blocks:
        native = vars(b)["forward"]
        assert isinstance(native, UNetResnet) and native.dtype == torch.bfloat16 and native.memory_format == torch.channels_last
        assert native.w1.shape == (native.cout, 9 * native.cin) and native.w1.dtype == torch.bfloat16
        assert torch.equal(native.w1.view(native.cout, 3, 3, native.cin), b.conv1.weight.permute(0, 2, 3, 1))
        assert native.w2.dtype == torch.bfloat16 and native.wt.dtype == torch.bfloat16 and torch.equal(native.wt, b.time_emb_proj.weight)
        assert (native.ws is not None) == (b.conv_shortcut is not None) and (native.ws is None or native.ws.dtype == torch.bfloat16)
        assert native.cb1.dtype == torch.float32 and torch.equal(native.cb1, b.conv1.bias.float())
        assert native.g1.dtype == torch.float32 and torch.equal(native.g1, b.norm1.weight.float())
    assert unpatch_unet_resnets(tree) == 2
    assert not any("forward" in vars(m) for m in tree.modules())


def test_a_block_of_the_other_type_is_refused_by_name():
    from fresco_amd import patch_unet_resnets
    tree = _tree()
    tree.up["resnets"][0].half()                      # one fp16 block in the bf16 tree
    with pytest.raises(NotImplementedError, match="bf16 blocks only") as e:
        patch_unet_resnets(tree, dtype=torch.bfloat16)
    assert "up.resnets.0" in str(e.value) and "torch.float16" in str(e.value)
    assert not any("forward" in vars(m) for m in tree.modules())     # ... before anything is patched
    # and the bf16 tree under the default dtype keeps the fp16 sentence
    with pytest.raises(NotImplementedError, match="fp16 blocks only") as e:
        patch_unet_resnets(_tree())
    assert "down.0" in str(e.value)
    with pytest.raises(TypeError, match="torch.float16 or torch.bfloat16"):
        patch_unet_resnets(_tree(), dtype=torch.float32)


def test_call_and_operator_type_checks():
    from fresco_amd import FrescoHipError, UNetResnet, ops
    from fresco_amd.vae import pack_conv_weight
    net = B.build(64, 128, torch.bfloat16)
    r = UNetResnet.from_module(net, dtype=torch.bfloat16)
    assert r.ws.shape == (128, 64) and r.ws.dtype == torch.bfloat16
    with pytest.raises(TypeError, match="bf16 parameters only"):
        UNetResnet(B.build(64, 128, torch.float16).state_dict(), "", 64, 128, dtype=torch.bfloat16)
    with pytest.raises(TypeError, match="bf16 x only"):
        r(torch.zeros(1, 64, 4, 4, dtype=torch.float16), torch.zeros(1, M.TEMB_CHANNELS, dtype=torch.bfloat16))
    with pytest.raises(TypeError, match="bf16 temb only"):
        r(torch.zeros(1, 64, 4, 4, dtype=torch.bfloat16), torch.zeros(1, M.TEMB_CHANNELS, dtype=torch.float16))
    with pytest.raises(FrescoHipError, match="GPU only"):   # no fallback on CPU tensors
        r(torch.zeros(1, 64, 4, 4, dtype=torch.bfloat16), torch.zeros(1, M.TEMB_CHANNELS, dtype=torch.bfloat16))
    # the operators: the element type is x's; another 16-bit type among the operands names both; fp32 still raises
    x = torch.zeros(1, 4, 4, 64, dtype=torch.bfloat16)
    w16 = pack_conv_weight(torch.zeros(64, 64, 3, 3))
    wbf = pack_conv_weight(torch.zeros(64, 64, 3, 3), dtype=torch.bfloat16)
    assert w16.dtype == torch.float16 and wbf.dtype == torch.bfloat16 and wbf.shape == (64, 576)
    with pytest.raises(TypeError, match="pack_conv_weight"):
        pack_conv_weight(torch.zeros(64, 64, 3, 3), dtype=torch.float32)
    with pytest.raises(TypeError, match=r"torch\.float16.*torch\.bfloat16"):
        ops.vae_conv(x, w16, None, 1, 4, 4, 64, 64, 3)
    with pytest.raises(TypeError, match=r"torch\.bfloat16.*torch\.float16"):
        ops.vae_conv(x.half(), wbf, None, 1, 4, 4, 64, 64, 3)
    with pytest.raises(TypeError, match=r"residual.*torch\.float16.*torch\.bfloat16"):
        ops.vae_conv(x, wbf, None, 1, 4, 4, 64, 64, 3, residual=x.half())
    with pytest.raises(TypeError, match=r"out.*torch\.float16.*torch\.bfloat16"):
        ops.vae_conv(x, wbf, None, 1, 4, 4, 64, 64, 3, out=x.half())
    with pytest.raises(TypeError):
        ops.vae_conv(x.float(), wbf, None, 1, 4, 4, 64, 64, 3)
    with pytest.raises(TypeError, match=r"torch\.float16.*torch\.bfloat16"):
        ops.conv_rows(x, torch.zeros(32, 64, dtype=torch.float16))
    with pytest.raises(TypeError):
        ops.unet_groupnorm(x.float(), torch.ones(64), torch.zeros(64))
    with pytest.raises(TypeError, match=r"weight.*torch\.float16.*torch\.bfloat16"):
        ops.unet_temb(torch.zeros(2, 64, dtype=torch.bfloat16), torch.zeros(8, 64, dtype=torch.float16), torch.zeros(8), torch.zeros(8))
    with pytest.raises(TypeError):
        ops.unet_temb(torch.zeros(2, 64), torch.zeros(8, 64), torch.zeros(8), torch.zeros(8))
    for call in (lambda: ops.vae_conv(x, wbf, None, 1, 4, 4, 64, 64, 3),
                 lambda: ops.unet_groupnorm(x, torch.ones(64), torch.zeros(64)),
                 lambda: ops.unet_temb(torch.zeros(2, 64, dtype=torch.bfloat16), torch.zeros(8, 64, dtype=torch.bfloat16),
                                       torch.zeros(8), torch.zeros(8))):
        with pytest.raises(FrescoHipError, match="GPU only"):
            call()


def test_the_record_is_current_and_holds_what_the_gpu_test_relies_on():
    import numpy as np
    gold = B.load_golden(os.path.join(ROOT, "tests", "golden"))
    assert sorted(gold) == sorted(B.case_key(c) + s for c in B.CASES for s in ("_tap", "_out", "_noise", "_peak"))
    case = B.CASES[-1]  # (640, 1280, 1, 4, 4): the cheapest to derive again
    key = B.case_key(case)
    tap, out, noise, peaks = B.record(case)
    np.testing.assert_allclose(gold[key + "_tap"], B.thin(tap), rtol=0, atol=1e-9)
    np.testing.assert_allclose(gold[key + "_out"], B.thin(out), rtol=0, atol=1e-9)
    np.testing.assert_allclose(gold[key + "_noise"], noise, rtol=1e-3)
    np.testing.assert_allclose(gold[key + "_peak"], peaks, rtol=1e-9)
    for c in B.CASES:
        k = B.case_key(c)
        # bf16 keeps 8 significant bits where fp16 keeps 11: the noise is positive and of that class
        assert gold[k + "_noise"].shape == (2,) and (gold[k + "_noise"] > 0).all() and (gold[k + "_noise"] < 2e-2).all()
        x, temb = B.inputs(c)
        assert x.dtype == temb.dtype == torch.bfloat16 and x.shape == (c[2], c[0], c[3], c[4])


# ---------------------------------------------------------------------------------------------------------------------
# 3. the listing of net_bf16.hip
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    if shutil.which(HIPCC) is None:
        pytest.skip("hipcc not found")
    out = str(tmp_path_factory.mktemp("net_bf16") / "net_bf16.s")
    subprocess.run([HIPCC] + FLAGS + [os.path.join(CSRC, "net_bf16.hip"), "-o", out], check=True, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL, timeout=900)
    text = open(out).read()
    kernels = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:", text, re.S):
        blk = m.group(0)
        g = lambda k: re.search(r"\." + k + r":\s+(\S+)", blk).group(1)  # noqa: E731
        kernels[g("name")] = dict(spill=int(g("vgpr_spill_count")), sgpr_spill=int(g("sgpr_spill_count")),
                                  scratch=int(g("private_segment_fixed_size")), lds=int(g("group_segment_fixed_size")),
                                  vgpr=int(g("vgpr_count")), agpr=int(g("agpr_count")), threads=int(g("max_flat_workgroup_size")))
    return text, kernels


def test_exactly_the_bf16_twins_exist_within_the_fp16_kernels_budgets(listing):
    _, kernels = listing
    assert all("DF16b" in n for n in kernels), sorted(kernels)         # every kernel of the file is a bf16 instantiation
    conv = sorted(n for n in kernels if "vae_conv_kernel" in n)
    assert len(conv) == 2 and any("ILi9E" in n for n in conv) and any("ILi1E" in n for n in conv), conv
    gn = ("unet_gn_lds_kernel", "unet_gn_stats_kernel", "unet_gn_finish_kernel", "unet_gn_apply_kernel")
    for pat in gn:
        assert len([n for n in kernels if pat in n]) == 1, (pat, sorted(kernels))
    temb = sorted(n for n in kernels if "unet_temb_kernel" in n)
    assert len(temb) == 4 and all(any("ILi%dE" % t in n for n in temb) for t in (1, 2, 3, 4)), temb
    assert len(kernels) == 2 + 4 + 4, sorted(kernels)
    for n, r in kernels.items():
        assert r["spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (n, r)
        assert r["vgpr"] * (r["threads"] // 64) <= 4 * 512, (n, r)
    for n in conv:   # tests/test_kernel_resources_vae.py's bar: two workgroups per CU
        assert kernels[n]["agpr"] <= kernels[n]["vgpr"] <= 256 and kernels[n]["threads"] == 256, (n, kernels[n])
    for pat in ("unet_gn_lds_kernel", "unet_gn_stats_kernel", "unet_gn_apply_kernel"):   # test_kernel_resources_unet.py's
        r = [r for n, r in kernels.items() if pat in n][0]
        assert r["threads"] == 512 and r["vgpr"] <= 128, (pat, r)


def test_lds_is_the_fp16_kernels(listing):
    _, kernels = listing
    lds = lambda pat: [r["lds"] for n, r in kernels.items() if pat in n]  # noqa: E731
    pair_sums, group_sums = 2 * 512 * 4 * 8, 2 * 32 * 8
    assert lds("vae_conv_kernel") == [0, 0]                                       # dynamic, 40 KiB, as vae.hip's
    assert lds("unet_gn_lds_kernel") == [pair_sums + group_sums + 2 * 32 * 4]
    assert lds("unet_gn_stats_kernel") == [pair_sums + group_sums]
    assert lds("unet_gn_apply_kernel") == [0] and lds("unet_gn_finish_kernel") == [0]
    assert lds("unet_temb_kernel") == [16 * 512 * 4] * 4
    src = open(os.path.join(CSRC, "net_bf16.hip")).read()
    assert "constexpr int NB_CONV_LDS = 2 * VC_A_BYTES + 2 * CT_B_BYTES;" in src and src.count("NB_CONV_LDS, st, a)") == 2
    assert src.count("allow_dyn_lds(unet_gn_lds_bf16_kernel, plane)") == 1


def test_the_text_is_bf16_without_atomics(listing):
    text, _ = listing
    assert "v_mfma_f32_32x32x16_bf16" in text and "global_load_lds_dwordx4" in text
    assert not re.search(r"v_mfma\w*_f16", text)
    assert "v_add_f64" in text and "v_fma_f64" in text                           # the statistics stay fp64
    assert "global_atomic" not in text and "flat_atomic" not in text and "ds_add" not in text
