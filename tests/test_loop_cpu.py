"""The denoising loop without a GPU: tests/loop_model.py's restatement of inference() + step() against the float64 record of
the unmodified reference (tests/golden/make_loop_golden.py), the restated tensor2numpy against its recorded table over every
fp16 bit pattern, the refusals of loop_update / loop_image_to_frames (fake pointers: every check answers before any HIP call),
and the signature of fresco_amd.inference against the reference's."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

import loop_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def lg():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", M.GOLDEN_FILE)))


def run_model(lg, name, monkeypatch, warp_tensor=None):
    pipe = M.Pipe("cpu", torch.float64)
    (imgs, embeds, edges), kw = M.make_inputs(name, "cpu", torch.float64)
    records = [torch.from_numpy(r) for r in lg[name + "_rec_in"]] if name + "_rec_in" in lg else []
    monkeypatch.setattr(torch, "randn", M.replay_randn(lg[name + "_draws"]))
    final = M.inference_model(pipe, pipe.controlnet, pipe.frescoProc, imgs, embeds, edges, pipe.scheduler.timesteps,
                              record_latents=records, warp_tensor=warp_tensor, **kw)
    steps = torch.stack([x[:M.CASES[name][0]] for x in pipe.unet.inputs])
    return pipe, steps, final, records


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_restatement_is_the_reference_in_float64(lg, name, monkeypatch):
    """cases without smoothing are the same float64 operations: 1e-12 of the peak.  With smoothing the injected
    oracle.fresco_oracle.warp_tensor and the reference's both compute in fp32 inside the float64 loop, about 6e-8 relative
    per step: 1e-5 leaves two orders of margin and stays fifty times under the fp16 noise the GPU bar rests on."""
    from oracle import fresco_oracle as O
    smooth = "smoothing" in M.CASES[name][1]
    pipe, steps, final, records = run_model(lg, name, monkeypatch, O.warp_tensor if smooth else None)
    peak = float(lg[name + "_peak"][0])
    assert peak == max(np.abs(lg[name + "_steps"]).max(), np.abs(lg[name + "_final"]).max())
    bound = (1e-5 if smooth else 1e-12) * peak
    d_steps = float((steps - torch.from_numpy(lg[name + "_steps"])).abs().max())
    d_final = float((final - torch.from_numpy(lg[name + "_final"])).abs().max())
    d_rec = float((torch.stack(records) - torch.from_numpy(lg[name + "_rec"])).abs().max())
    print("%s: steps %.2e final %.2e records %.2e of bound %.2e" % (name, d_steps, d_final, d_rec, bound))
    assert d_steps <= bound and d_final <= bound and d_rec <= bound
    assert M.finish_trace(pipe.trace) + pipe.progress == json.loads(str(lg[name + "_trace"]))
    assert float(lg[name + "_noise"][0]) > 50 * 1e-5 or not smooth


def test_the_record_covers_what_the_loop_branches_on(lg):
    tr = {n: json.loads(str(lg[n + "_trace"])) for n in M.CASES}
    assert [e[1] for e in tr["warm2"] if e[0] == "unet"] == M.STEPS[2:]
    assert [e[1] for e in tr["warmneg"] if e[0] == "unet"] == M.STEPS
    assert [e[2] for e in tr["warm2"] if e[0] == "controlnet"] == M.COND_SCALE[2:]
    assert not [e for e in tr["nocn"] if e[0] == "controlnet"]
    # disable_intraattn from the second step on, disable_interattn at 301 and 151, in that order within a step
    assert tr["warm0"].count(["disable_intraattn"]) == 5 and tr["warm0"].count(["disable_interattn"]) == 2
    k = tr["warm0"].index(["disable_interattn"])
    assert tr["warm0"][k - 1] == ["disable_intraattn"] and tr["warm0"][k + 1][:2] == ["controlnet", 301]
    assert ["total", 4] in tr["warm2"] and tr["warm2"].count(["update"]) == 4
    # restore before record: a propagation batch's record row 0 is the row it was handed
    assert np.array_equal(lg["prop_rec"][:, 0], lg["prop_rec_in"][:, 0])
    assert np.array_equal(lg["prop_rec_in"], lg["first_rec"])
    assert not np.array_equal(lg["prop_rec"][:, 1], lg["prop_rec_in"][:, 1])
    assert np.array_equal(lg["prop2_rec"], lg["prop2_rec_in"])  # two frames: both rows are restored rows
    # repeat_noise reaches the initial latents only: equal frames before the SDEdit start, independent noise after
    assert len(lg["first_draws"]) == 6 and not np.array_equal(lg["first_draws"][1][0], lg["first_draws"][1][1])
    assert not np.array_equal(lg["first_final"][0], lg["first_final"][1])


def test_uint8_table_is_the_restated_expression(lg):
    keep = ~lg["u8_nan"]
    assert lg["u8_nan"].sum() == 2 * 1023 and lg["u8_table"].dtype == np.uint8
    got = M.image_to_frames_model(M.all_half_patterns()).reshape(-1)
    assert np.array_equal(got[keep], lg["u8_table"][keep])
    assert got.shape == (65536,) and set(np.unique(lg["u8_table"][keep])) == set(range(256))


@pytest.fixture(scope="module")
def lib():
    from fresco_amd import _lib
    return _lib.load()


def test_loop_update_refusals(lib):
    from fresco_amd import _lib
    p = 4096  # fake, never touched

    def call(xt=p, eps=p, x0_in=None, noise=p, restore=None, out=p, model_input=p, record=p, frames=3, frame_elems=256,
             text_offset=768, noise_period=768, copies=2, sqrt_alpha=0.5, dtype=_lib.F16):
        return lib.loop_update(xt, eps, x0_in, noise, restore, out, model_input, record, frames, frame_elems, text_offset,
                               noise_period, copies, 7.5, 0.5, sqrt_alpha, 0.5, 0.5, 0.5, dtype, None)

    assert call(xt=None) == EINVAL and call(noise=None) == EINVAL and call(out=None) == EINVAL
    assert call(eps=None) == EINVAL                      # neither eps nor x0_in
    assert call(restore=p, frames=1) == EINVAL           # the reference's latents[0:2] = ... fails there
    for bad in (dict(frames=0), dict(frames=-1), dict(frame_elems=0), dict(noise_period=0), dict(text_offset=-1),
                dict(copies=0), dict(copies=3), dict(sqrt_alpha=0.0), dict(sqrt_alpha=float("nan"))):
        assert call(**bad) == EINVAL, bad
    for code in (3, -1, 99):
        assert call(dtype=code) == EUNSUPPORTED
    assert call(frames=1 << 20, frame_elems=1 << 19) == EUNSUPPORTED
    assert call(xt=None, dtype=99) == EINVAL             # argument checks come first


def test_loop_image_to_frames_refusals(lib):
    from fresco_amd import _lib
    p = 4096

    def call(x=p, out=p, n=2, C=3, H=5, W=7, dtype=_lib.F16):
        return lib.loop_image_to_frames(x, out, n, C, H, W, dtype, None)

    assert call(x=None) == EINVAL and call(out=None) == EINVAL
    for bad in (dict(n=0), dict(C=0), dict(H=-1), dict(W=0)):
        assert call(**bad) == EINVAL, bad
    assert call(dtype=_lib.BF16) == EUNSUPPORTED         # the reference's .numpy() raises on bf16
    assert call(dtype=7) == EUNSUPPORTED
    assert call(C=5) == EUNSUPPORTED
    assert call(n=1 << 10, H=1 << 15, W=1 << 15) == EUNSUPPORTED


def test_a_library_without_the_loop_symbols_is_refused_by_name(lib, monkeypatch):
    from fresco_amd import _lib

    class Older:
        def __getattr__(self, name):
            if name.startswith("loop_"):
                raise AttributeError(name)
            return getattr(lib, name)

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib.ctypes, "CDLL", lambda path: Older())
    with pytest.raises(_lib.FrescoHipError, match="does not export loop_update"):
        _lib.load()
    assert set(_lib.LOOP_SIGNATURES) == {"loop_update", "loop_image_to_frames"}
    header = open(os.path.join(ROOT, "include", "fresco_loop.h")).read()
    assert "int loop_update(" in header and "int loop_image_to_frames(" in header and "fresco_loop" not in \
        open(os.path.join(ROOT, "include", "fresco_hip.h")).read()


def test_signature_is_the_references(lg):
    import fresco_amd
    sig = inspect.signature(fresco_amd.inference)
    assert list(sig.parameters) == [str(n) for n in lg["sig_names"]]
    ours = ["<none>" if p.default is inspect.Parameter.empty else repr(p.default) for p in sig.parameters.values()]
    assert ours == [str(d) for d in lg["sig_defaults"]]
    assert all(p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for p in sig.parameters.values())
    assert fresco_amd.tensor2numpy is fresco_amd.loop.tensor2numpy and "inference" in fresco_amd.__all__
    with pytest.raises(NotImplementedError):
        fresco_amd.inference(None, None, None, None, None, None, None, visualize_pipeline=True)


def test_hook_latch_prefers_the_host_timestep():
    """fresco_amd.inference hands the step's host integer over; the latch then never converts its (device) argument"""
    from fresco_amd.hook import _OptState

    class Unreadable:
        def __int__(self):
            raise AssertionError("the latch read the timestep it was handed")

    st = _OptState([901, 601], [], None, None, [], 1e2, 20, True, None)
    st.host_timestep = 601
    st.latch(Unreadable())
    assert st.active and st.host_timestep is None
    st.host_timestep = 751
    st.latch(Unreadable())
    assert not st.active
    st.latch(torch.tensor(901))  # without a hand-over: as before
    assert st.active
    with pytest.raises(AssertionError):
        st.latch(Unreadable())
