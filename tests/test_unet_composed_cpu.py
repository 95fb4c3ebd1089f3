"""The composed stand-in UNet + ControlNet (tests/unet_composed_model.py) without a GPU: what the models hold (every kind of
site, the parameter budget, diffusers' names, the processor table), the golden file against a fresh derivation, and that the
record can tell the faults of a composition apart: each planted fault moves the float64 model away from the record by at
least twice the bar the GPU tests hold the native path to (4 x noise x peak).  The same for the second file: the store pass,
the call with the spatial-guided pass and the controller's sequence through four steps of the loop."""
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


# ---------------------------------------------------------------------------------------------------------------------
# the store pass, the spatial-guided call and the controller's sequence (unet_composed_seq_golden.npz)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seq_gold():
    return M.seq_golden(GOLDEN)


def test_seq_golden_file_is_current(models, seq_gold):
    fresh = M.derive_seq(models, draws=list(seq_gold["seq_draws"]))
    assert sorted(seq_gold) == sorted(fresh)
    assert os.path.getsize(os.path.join(GOLDEN, M.SEQ_GOLDEN_FILE)) < (1 << 20)
    for k in sorted(seq_gold):
        if k.endswith("_noise"):
            np.testing.assert_allclose(seq_gold[k], fresh[k], rtol=0.25, err_msg=k)      # (as test_golden_file_is_current)
            assert (seq_gold[k] > 0).all() and (seq_gold[k] < 1e-2).all(), k
        else:
            np.testing.assert_allclose(seq_gold[k], fresh[k], rtol=0, atol=1e-9, err_msg=k)
    assert seq_gold["seq_steps"].shape == (4, M.FRAMES, 4, M.LAT, M.LAT) and seq_gold["seq_draws"].shape[0] == 5
    assert seq_gold["store_attn0"].shape[0] == seq_gold["store_attn1"].shape[0] == 2 * M.FRAMES
    # the Gram targets of 2 x 2 and 4 x 4 planes whole; 64 rows at every 3rd (0 .. 63), 256 at every 10th plus the last
    assert [seq_gold["store_gram%d" % i].shape[1] for i in range(4)] == [4, 16, 22, 27]


def test_the_seq_cases_are_apart(gold, seq_gold):
    """the spatial-guided pass was live; the loop moved; the store pass ran on other latents than the later call; the
    controller went through the reference's sequence with its index back at 0 at every call"""
    bar = 4 * float(seq_gold["full_noise"][0]) * float(seq_gold["full_peak"][0])
    assert M.distance(seq_gold["full_out"], gold["fresco_out"]) > 2 * bar
    s = seq_gold["seq_steps"]
    bar = 4 * float(seq_gold["seq_noise"][0]) * float(seq_gold["seq_peak"][0])
    assert all(M.distance(s[i], s[j]) > 2 * bar for i in range(4) for j in range(i + 1, 4))
    assert tuple(map(tuple, seq_gold["seq_flags"].tolist())) == M.SEQ_FLAGS
    x, _, _, _ = M.call_inputs()
    assert M.distance(M.store_latents(torch.float64), x.double()) > 1.0


def test_the_restated_controller_follows_control_py():
    """Fresco's store, read index and switches against fresco_amd.control.AttentionControl, call for call"""
    from fresco_amd.control import AttentionControl
    ctrl, f = AttentionControl(), M.make_fresco(torch.float64)
    f.disable_controller()
    state = lambda: (int(ctrl.use_intraattn), int(ctrl.use_interattn), int(ctrl.use_cfattn), ctrl.index)  # noqa: E731
    ctrl.enable_intraattn(), f.enable_intraattn()              # an empty store: both stay off
    assert state() == f.flags() == (0, 0, 0, 0)
    ctrl.enable_store(), f.enable_store()
    for i in range(3):
        ctrl(torch.full((1,), float(i)))
        f.stored.append(torch.full((1,), float(i)))
    ctrl.enable_intraattn(), f.enable_intraattn()
    assert not ctrl.store and not f.store and state() == f.flags() == (1, 0, 0, 0)
    for i in range(7):                                         # two cycles and one more
        assert float(ctrl(None)) == float(f.read()) == i % 3 and ctrl.index == f.index == (i + 1) % 3
    ctrl.disable_intraattn(), f.disable_intraattn()
    assert state() == f.flags() == (0, 0, 0, 0) and len(f.stored) == len(ctrl.stored_attn["decoder_attn"]) == 3
    ctrl.clear_store(), f.clear_store()
    assert f.stored == [] and ctrl.stored_attn["decoder_attn"] == []


@pytest.mark.parametrize("fault", M.FULL_FAULTS + M.SEQ_FAULTS + M.GRAM_FAULTS)
def test_the_seq_record_tells_the_fault(fault, models, gold, seq_gold):
    d, bar = M.seq_fault_distance(models, fault, seq_gold)
    print("%s: %.4g from the record = %.2f bars (bar %.4g)" % (fault, d, d / bar, bar))
    assert d >= 2 * bar, (fault, d, bar)
    if fault == M.GRAM_FAULTS[-1]:      # the models are as they were: `plain` is its record again
        r64, _ = models.call("plain", fault=None)
        np.testing.assert_allclose(r64["out"], gold["plain_out"], rtol=0, atol=1e-9)
