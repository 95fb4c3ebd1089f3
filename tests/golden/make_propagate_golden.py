"""Generate tests/golden/propagate_golden.npz: the reference's own Ebsynth stage of video_blend.py
(process_one_sequence with the blender.guide classes, unmodified) on a tiny synthetic video, with the stand-ins of
tests/video_blend_standins.py for cv2, flow_calc.get_flow and the Ebsynth process.

The reference is imported through _ref_harness.py's recipe, plus stubs for what it does not cover: numba's njit as the
identity, src.video_util (absent from the tree), and flow.flow_utils loaded with FlowCalc's model construction stood in
(GMFlow a placeholder, no checkpoint read); flow_calc.get_flow is then the stand-in's, while flow_calc.warp and
flow_warp run as the reference's own code on CPU.  PositionalGuide's ./guide/<k>.jpg debug masks go to a scratch
working directory and are not recorded.

Video: tests/video_blend_standins.make_video, key frames KEY_IND = [0, 3, 7] (intervals 3 and 4, both directions).
Recorded: every Ebsynth argv (paths relative to the video's base directory, keyed by output), and every file the stage
writes under the base directory except flows: guides and outputs as decoded pixels, .bin files as bytes.

Run:  python tests/golden/make_propagate_golden.py
"""
import contextlib
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, TESTS)
sys.path.insert(0, os.path.dirname(TESTS))
import _ref_harness as H  # noqa: E402
import video_blend_standins as S  # noqa: E402

OUT = os.path.join(HERE, "propagate_golden.npz")


def _stub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


class _GMFlowPlaceholder:
    def __init__(self, **kw):
        pass

    def to(self, *a, **kw):
        return self

    def load_state_dict(self, *a, **kw):
        return None

    def eval(self):
        return self


@contextlib.contextmanager
def _cwd(path):
    old = os.getcwd()
    os.chdir(path)
    try:
        yield
    finally:
        os.chdir(old)


def load_video_blend():
    """the reference's video_blend module, with cv2 = the stand-in and flow_calc.get_flow = the stand-in"""
    if not H.reference_available():
        raise RuntimeError("the reference tree is not present")
    sys.dont_write_bytecode = True
    cv2 = _stub("cv2", **vars(S.cv2))
    _stub("numba", njit=lambda f: f)
    _stub("src.video_util", frame_to_video=lambda *a, **kw: None)
    _stub("gmflow")
    _stub("gmflow.gmflow", GMFlow=_GMFlowPlaceholder)
    _stub("utils")
    _stub("utils.utils", InputPadder=object)
    load = torch.load
    torch.load = lambda *a, **kw: {}
    try:
        with _cwd(H.REF_ROOT):
            for p in (H.REF_ROOT, os.path.join(H.REF_ROOT, "src", "ebsynth")):
                if p not in sys.path:
                    sys.path.insert(0, p)
            import video_blend as vb
    finally:
        torch.load = load
    fu = sys.modules["flow.flow_utils"]
    assert vb.flow_calc is fu.flow_calc and vb.cv2 is cv2
    fu.flow_calc.get_flow = S.get_flow
    return vb


def run_reference(vb, base):
    S.make_video(base, S.KEY_IND)
    vs = S.VideoSequence(base, S.KEY_IND)
    sub = S.SubprocessStandin()
    vb.subprocess = sub
    work = tempfile.mkdtemp()
    os.makedirs(os.path.join(work, "guide"))
    with _cwd(work):
        for i in range(vs.n_seq):
            vb.process_one_sequence(i, vs)
    return sub.argvs


def main():
    vb = load_video_blend()
    base = os.path.join(tempfile.mkdtemp(), "run")
    argvs = run_reference(vb, base)
    argv_by_output = {os.path.relpath(a[a.index("-output") + 1], base): S.relative_argv(a, base) for a in argvs}
    files = S.snapshot(base)
    arrays = {"file:" + k.replace(os.sep, "|"): v for k, v in files.items()}
    np.savez_compressed(OUT, argv=np.array(json.dumps(argv_by_output, sort_keys=True)),
                        inputs_sha256=np.array(S.inputs_digest(base)), **arrays)
    print("wrote %s: %d commands, %d files, %d bytes" % (OUT, len(argvs), len(files), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
