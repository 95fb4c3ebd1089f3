"""The composed stand-in UNet + ControlNet (tests/unet_composed_model.py) without a GPU: what the models hold (every kind of
site, the parameter budget, diffusers' names, the processor table), the golden file against a fresh derivation, and that the
record can tell the faults of a composition apart: each planted fault moves the float64 model away from the record by at
least twice the bar the GPU tests hold the native path to (4 x noise x peak)."""
import os

import numpy as np
import pytest
import torch

import unet_composed_model as M
import unet_resnet_model as R
import unet_shell_model as S
import unet_transformer_model as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def models():
    return M.Models()


@pytest.fixture(scope="module")
def gold():
    return M.load_golden(GOLDEN)


@pytest.fixture(scope="module")
def fresh(models, gold):
    """every record derived again, once, with the recorded draws replayed"""
    return M.derive(models, draws=list(gold["loop_draws"]))


def test_the_models_hold_every_kind_of_site(models):
    u, c = models.u64, models.c64
    assert M.parameters_of(u) + M.parameters_of(c) <= M.PARAM_LIMIT
    assert len(u.up_blocks) == 4 and len(u.down_blocks) == 4
    width = lambda blk: blk.resnets[-1].conv2.out_channels  # noqa: E731
    assert [width(b) for b in u.up_blocks] == [1280, 640, 640, 320]
    resnets = {(m.conv1.in_channels, m.conv1.out_channels) for net in (u, c) for m in net.modules() if isinstance(m, R.Resnet)}
    cats = {(m.conv1.in_channels, m.conv1.out_channels) for b in u.up_blocks for m in b.resnets}
    assert {(640, 320), (960, 640), (1920, 1280)} <= cats and cats <= resnets
    tfs = {m.proj_in.in_channels for m in u.modules() if isinstance(m, T.Transformer)}
    assert tfs == {320, 640, 1280}
    assert {m.channels for m in u.modules() if isinstance(m, S.Downsample2D)} == {320, 640}
    assert {m.channels for m in u.modules() if isinstance(m, S.Upsample2D)} == {1280, 640}
    assert len(c.controlnet_down_blocks) == 5 and c.controlnet_mid_block.out_channels == 1280
    assert isinstance(c.controlnet_cond_embedding, S.CondEmbedding)
    for name in ("conv_in", "time_proj", "time_embedding", "conv_norm_out", "conv_act", "conv_out"):
        assert hasattr(u, name)
    # head dims 40, 80 and 160: the three dispatch branches of the attention processors
    assert {m.to_q.out_features // m.heads for _, m in u._attention_modules()} == {40, 80, 160}


def test_the_processor_table_follows_diffusers_names(models):
    u, c = models.u64, models.c64
    keys = list(u.attn_processors)
    assert len(keys) == 12 and all(k.endswith((".attn1.processor", ".attn2.processor")) for k in keys)
    assert "up_blocks.2.attentions.0.transformer_blocks.0.attn1.processor" in keys
    assert "mid_block.attentions.0.transformer_blocks.0.attn2.processor" in keys
    assert sorted(M.fresco_names(u)) == sorted(k[:-len(".processor")] for k in keys if k.startswith(("up_blocks.2", "up_blocks.3")))
    assert len(M.fresco_names(u)) == 6 and len(c.attn_processors) == 6 and not M.fresco_names(c)
    marker, before = object(), dict(u.attn_processors)
    u.set_attn_processor({k: (marker if k.startswith("up_blocks.3") else v) for k, v in before.items()})
    assert [k for k, v in u.attn_processors.items() if v is marker] == [k for k in keys if k.startswith("up_blocks.3")]
    u.set_attn_processor(before)
    assert dict(u.attn_processors) == before
    models.reset()


def test_golden_file_is_current(gold, fresh):
    assert sorted(gold) == sorted(fresh)
    for k in sorted(gold):
        if k.endswith("_noise"):
            # a maximum over fp32 runs whose sums depend on the CPU's order of additions (unet_shell's golden test: some per
            # cent between CPUs); the tests use it under a margin of 4
            np.testing.assert_allclose(gold[k], fresh[k], rtol=0.25, err_msg=k)
            assert (gold[k] > 0).all() and (gold[k] < (5e-2 if k.startswith("bf16") else 1e-2)).all(), k
        else:
            np.testing.assert_allclose(gold[k], fresh[k], rtol=0, atol=1e-9, err_msg=k)
    assert gold["loop_steps"].shape == (3, M.FRAMES, 4, M.LAT, M.LAT) and gold["loop_draws"].shape[0] == 4
    assert gold["plain_out"].shape == (2 * M.FRAMES, 4, M.LAT, M.LAT)


def test_the_cases_are_apart(gold):
    """fresco's sites were live; an edit of the edges or of the text shows: each by more than twice plain's bar"""
    bar = 4 * float(gold["plain_noise"][0]) * float(gold["plain_peak"][0])
    for case in ("fresco", "halfedges", "halftext"):
        assert M.distance(gold[case + "_out"], gold["plain_out"]) > 2 * bar, case
    # the loop moved: three different UNet inputs
    s = gold["loop_steps"]
    loop_bar = 4 * float(gold["loop_noise"][0]) * float(gold["loop_peak"][0])
    assert M.distance(s[0], s[1]) > 2 * loop_bar and M.distance(s[1], s[2]) > 2 * loop_bar


@pytest.mark.parametrize("fault", M.FAULTS)
def test_the_record_tells_the_fault(fault, models, gold, fresh):
    d, bar = M.fault_distance(models, fault, gold)
    print("%s: %.4g from the record = %.2f bars (bar %.4g)" % (fault, d, d / bar, bar))
    assert d >= 2 * bar, (fault, d, bar)
    # and the models are as they were: the unfaulted run is the record again
    if fault == M.FAULTS[-1]:
        r64, _ = models.call("plain", fault=None)
        np.testing.assert_allclose(r64["out"], gold["plain_out"], rtol=0, atol=1e-9)
