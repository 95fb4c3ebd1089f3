"""fresco_amd.propagate (video_blend.py's Ebsynth stage in one process) on the GPU.

1. Against the unmodified reference: tests/golden/propagate_golden.npz (make_propagate_golden.py) holds what the
   reference's process_one_sequence and guide classes wrote with the stand-ins of tests/video_blend_standins.py.  The
   driver runs with the same stand-ins and synthesis replaced by the same answering function: the composed argv of
   every frame, every guide file, every output and every .bin equal the golden.  (The reference's ./guide/ debug masks
   are the one documented gap.)
2. Against recipe C: the real batched synthesis (max_batch 1, 2 and the default) against a loop written here that
   builds the guides independently (numpy edge filter, torch-CPU nearest warp, the stand-in inpaint and codec) and
   runs the shim, fresco_amd.ebsynth.main(argv), in process per frame: decoded outputs and .bin files byte-equal.
"""
import json
import os
import sys
import types

import numpy as np
import pytest

from fresco_amd import ebsynth as E
from fresco_amd import propagate as P

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import video_blend_standins as S  # noqa: E402
from test_gpu_guides import edge_model, warp_model  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(HERE, "golden", "propagate_golden.npz")


@pytest.fixture
def guide_module(monkeypatch):
    """blender.guide as the driver finds it once video_blend.py is loaded, here with the stand-in read_flow /
    read_mask"""
    monkeypatch.setitem(sys.modules, "blender.guide",
                        types.SimpleNamespace(read_flow=S.read_flow, read_mask=S.read_mask))


def run_driver(base, **kw):
    S.make_video(base, S.KEY_IND)
    vs = S.VideoSequence(base, S.KEY_IND)
    vb = types.SimpleNamespace(cv2=S.cv2, flow_calc=types.SimpleNamespace(get_flow=S.get_flow))
    P.patch_run_ebsynth(vb, **kw)
    vb.run_ebsynth(vs)
    return vs


def assert_same_files(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def test_matches_the_reference_stage(tmp_path, guide_module, capsys):
    g = np.load(GOLDEN)
    base = str(tmp_path / "run")
    argvs = []

    def synth(jobs):
        argvs.extend(j["argv"] for j in jobs)
        return S.answer_all(jobs)

    run_driver(base, synth=synth)
    assert "ebsynth: " in capsys.readouterr().out
    assert S.inputs_digest(base) == str(g["inputs_sha256"])
    want_argv = json.loads(str(g["argv"]))
    got_argv = {os.path.relpath(a[a.index("-output") + 1], base): S.relative_argv(a, base) for a in argvs}
    assert len(argvs) == len(want_argv) == 10
    assert got_argv == want_argv
    want = {k[len("file:"):].replace("|", os.sep): g[k] for k in g.files if k.startswith("file:")}
    assert_same_files(S.snapshot(base), want)


# ---------------------------------------------------------------------------------------------------------------------
# recipe C: guides built here, the shim per frame
def first_positional(h, w):
    y = (np.linspace(0, 1, h)[:, None] * 255).astype(np.uint8) * np.ones((1, w), np.uint8)
    x = (np.linspace(0, 1, w)[None, :] * 255).astype(np.uint8) * np.ones((h, 1), np.uint8)
    return np.stack([np.zeros((h, w), np.uint8), x, y], -1)


def recipe_c(base):
    S.make_video(base, S.KEY_IND)
    vs = S.VideoSequence(base, S.KEY_IND)
    for i in range(vs.n_seq):
        for fwd in (True, False):
            n = vs.interval(i)
            inputs, outputs = vs.get_input_sequence(i, fwd), vs.get_output_sequence(i, fwd)
            flows, key = vs.get_flow_sequence(i, fwd), vs.get_key_img(i if fwd else i + 1)
            edges, temporal, pos = (vs.get_edge_sequence(i, fwd), vs.get_temporal_sequence(i, fwd),
                                    vs.get_pos_sequence(i, fwd))
            for j in range(n - 1):
                S.get_flow(S.imread(inputs[j]), S.imread(inputs[j + 1]), flows[j])
            fl = [np.load(f)[0] for f in flows]
            masks = [S.read_mask(f) for f in flows]
            for p, f in zip(edges, inputs):
                S.imwrite(p, edge_model(S.imread(f)))
            S.imwrite(temporal[0], S.imread(key))
            img = first_positional(*fl[0].shape[1:])
            S.imwrite(pos[0], img)
            for k in range(n - 1):
                img = S.inpaint(warp_model(img, fl[k]), masks[k], 30, S.INPAINT_TELEA)
                S.imwrite(pos[k + 1], img)
            S.imwrite(outputs[0], S.imread(key))
            for j in range(1, n):
                warped = warp_model(S.imread(outputs[j - 1]), fl[j - 1])
                S.imwrite(temporal[j], S.inpaint(warped, masks[j - 1], 30, S.INPAINT_TELEA))
                argv = ["-style", os.path.abspath(key)]
                for seq, w in ((inputs, "6"), (edges, "0.5"), (temporal, "0.5"), (pos, "2")):
                    argv += ["-guide", os.path.abspath(seq[0]), os.path.abspath(seq[j]), "-weight", w]
                argv += ["-output", os.path.abspath(outputs[j]), "-searchvoteiters", "12", "-patchmatchiters", "6"]
                assert E.main(argv) == 0


@pytest.fixture(scope="module")
def recipe_c_files(tmp_path_factory):
    base = str(tmp_path_factory.mktemp("recipe_c") / "run")
    recipe_c(base)
    return S.snapshot(base)


@pytest.mark.parametrize("max_batch", [1, 2, None])
def test_matches_recipe_c(tmp_path, guide_module, recipe_c_files, max_batch):
    base = str(tmp_path / "run")
    stats = {}
    run_driver(base, max_batch=max_batch, stats=stats)
    # steps 1 and 2 run all four chains, step 3 the two of the longer interval
    want_batches = {1: [1] * 10, 2: [2, 2, 2, 2, 2], None: [4, 4, 2]}[max_batch]
    assert stats["batches"] == want_batches
    assert_same_files(S.snapshot(base), recipe_c_files)
