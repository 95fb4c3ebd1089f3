"""video_blend.py's Ebsynth stage in one process: every key interval, both directions, through batched GPU synthesis.

The reference's ``run_ebsynth`` starts one Ebsynth process per in-between frame and direction (``process_one_sequence``
through ``subprocess.run``).  ``patch_run_ebsynth(vb)`` rebinds a loaded ``video_blend`` module's ``run_ebsynth`` to
``run_ebsynth`` here, which writes the same files:

* flows through the module's own ``flow_calc.get_flow`` (same arguments and save paths), or in one batched
  ``flow_calc.get_flows`` call over every chain's pairs when it has one (``fresco_amd.flowcalc.FlowCalc``, recipe E),
  read back through the ``read_flow`` / ``read_mask`` that ``blender.guide`` uses;
* the edge, positional and temporal guides and ``output_seq[0]`` through the module's own ``cv2`` (``imread``,
  ``imwrite``, ``inpaint(..., 30, INPAINT_TELEA)``); the edge filter and the nearest warps run on the GPU
  (``fresco_amd.ebsynth.edge_guide`` / ``warp_nearest``), inpainting stays on the host;
* every synthesis input is what recipe C's shim would read: the argv the reference composes goes through the shim's
  ``parse_cli``, each file named there is decoded with the shim's loader (so a lossy ``.jpg`` guide is seen as written)
  and packed by ``pack_inputs``; outputs are PNG content at each output path plus ``write_error_bin(bin_path(...))``.

Schedule: all chains' flows and positional guides first; then step j = 1, 2, ... runs every (interval, direction)
chain longer than j in lockstep (step j's temporal guide needs step j - 1's output), grouped by packed layout and
weights, in batches of at most ``max_batch`` problems, seed 0 each (as the shim).  ``--n_proc`` has no effect.

Departure: ``PositionalGuide`` also writes its masks to ``./guide/<k>.jpg`` under the working directory (debug output
that nothing reads); this driver does not.  DESIGN.md section 9, INTEGRATION.md recipe C.
"""
import os
import shlex
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import ebsynth as E

WEIGHTS = (6, 0.5, 0.5, 2)  # process_one_sequence: color, edge, temporal, positional
TAIL = " -searchvoteiters 12 -patchmatchiters 6"
WORKSPACE_BUDGET = 4 << 30  # default max_batch: as many problems as fit this much workspace (at most MAX_BATCH)
MAX_THREADS = 16


def first_positional_image(h, w):
    """PositionalGuide.__generate_first_img: float64 (h, w, 3) BGR, g / r = truncated 255 * linspace along x / y."""
    i, j = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    r = (i * 255).astype(np.uint8)
    g = (j * 255).astype(np.uint8)
    b = np.zeros(r.shape)
    return np.stack((b, g, r), 2)


def compose_cmd(key_img, guide_pairs, output, ebsynth_bin="ebsynth"):
    """process_one_sequence's command line for one frame: guide_pairs = [(source, target)] of the color, edge,
    temporal and positional guides, weighted 6 / 0.5 / 0.5 / 2."""
    cmd = f'{ebsynth_bin} -style {os.path.abspath(key_img)}'
    for (src, tgt), w in zip(guide_pairs, WEIGHTS):
        cmd += ' ' + f'-guide {os.path.abspath(src)} {os.path.abspath(tgt)} -weight {w}'
    cmd += f' -output {os.path.abspath(output)}' + TAIL
    return cmd


def compose_argv(key_img, guide_pairs, output):
    """The argv the shim receives for compose_cmd (the shell's split, program name dropped)."""
    return shlex.split(compose_cmd(key_img, guide_pairs, output))[1:]


class Chain:
    """One (interval, direction) of process_one_sequence: its paths, and per step its guides."""

    def __init__(self, vs, i, forward):
        self.i, self.forward = i, forward
        self.interval = vs.interval(i)
        self.inputs = vs.get_input_sequence(i, forward)
        self.outputs = vs.get_output_sequence(i, forward)
        self.flows = vs.get_flow_sequence(i, forward)
        self.key_img = vs.get_key_img(i if forward else i + 1)
        self.edges = vs.get_edge_sequence(i, forward)
        self.temporal = vs.get_temporal_sequence(i, forward)
        self.pos = vs.get_pos_sequence(i, forward)

    def guide_pairs(self, j):
        return [(s[0], s[j]) for s in (self.inputs, self.edges, self.temporal, self.pos)]

    def argv(self, j):
        return compose_argv(self.key_img, self.guide_pairs(j), self.outputs[j])


def steps(chains):
    """Lockstep schedule: [(j, [chain indices with interval > j])] for j = 1 .. max interval - 1."""
    top = max((c.interval for c in chains), default=0)
    return [(j, [k for k, c in enumerate(chains) if c.interval > j]) for j in range(1, top)]


def group_key(job):
    """Problems that can share one batched call: equal packed shapes, weights and per-call arguments."""
    cfg = job["cfg"]
    return (job["style"].shape, job["source_guide"].shape, job["target_guide"].shape, tuple(job["style_weights"]),
            tuple(job["guide_weights"]), cfg["uniformity"], cfg["patchsize"], cfg["pyramidlevels"],
            cfg["searchvoteiters"], cfg["patchmatchiters"], cfg["stopthreshold"], cfg["extrapass3x3"])


def batches(jobs, max_batch):
    """Group job indices by group_key (first-seen order) and cut each group into runs of at most max_batch (None:
    default_max_batch of the group's shapes)."""
    groups = {}
    for k, job in enumerate(jobs):
        groups.setdefault(group_key(job), []).append(k)
    out = []
    for idx in groups.values():
        mb = max_batch if max_batch is not None else default_max_batch(jobs[idx[0]])
        mb = max(1, min(int(mb), E.MAX_BATCH))
        out += [idx[s:s + mb] for s in range(0, len(idx), mb)]
    return out


def default_max_batch(job):
    """As many problems as fit WORKSPACE_BUDGET bytes of workspace, at most E.MAX_BATCH."""
    st, sg, tg = job["style"], job["source_guide"], job["target_guide"]
    one = E.batch_workspace_bytes(1, st.shape[2], sg.shape[2], st.shape[:2], tg.shape[:2], job["cfg"]["patchsize"])
    return max(1, min(E.MAX_BATCH, WORKSPACE_BUDGET // max(one, 1)))


def load_job(argv, cache=None):
    """What the shim does with argv before synthesis: parse_cli, decode every named file with its loader, check the
    sizes and pack.  `cache`: path -> decoded RGBA, for files that do not change during the run."""
    cfg = E.parse_cli(argv)

    def load(path):
        if cache is not None and path in cache:
            return cache[path]
        return E._load_rgba(path)

    style = load(cfg["style"])
    guides = [(load(s), load(t)) for s, t, _ in cfg["guides"]]
    for (s, t), (sn, tn, _) in zip(guides, cfg["guides"]):
        if s.shape[:2] != style.shape[:2]:
            raise E.CliError("source guide '%s' doesn't match the resolution of '%s'" % (sn, cfg["style"]))
        if t.shape[:2] != guides[0][1].shape[:2]:
            raise E.CliError("target guide '%s' doesn't match the resolution of '%s'" % (tn, cfg["guides"][0][1]))
    st, sg, tg, swt, gwt = E.pack_inputs(style, guides, cfg["style_weight"], [g[2] for g in cfg["guides"]])
    if st.shape[2] > E.MAX_STYLE_CHANNELS or sg.shape[2] > E.MAX_GUIDE_CHANNELS:
        raise E.CliError("too many channels (style %d, guide %d)" % (st.shape[2], sg.shape[2]))
    return dict(argv=list(argv), cfg=cfg, style=st, source_guide=sg, target_guide=tg, style_weights=swt,
                guide_weights=gwt)


def _device():
    return torch.device("cuda", torch.cuda.current_device())


def gpu_synth(jobs):
    """The default synthesis: one ebsynth_run_batch over jobs of one group_key, seed 0 each (the shim's).  Returns
    [(image uint8 (h, w, ns), error float32 (h, w))] on the host."""
    dev = _device()
    cfg = jobs[0]["cfg"]

    def stack(key):
        return torch.from_numpy(np.stack([j[key] for j in jobs])).to(dev)

    img, err = E.ebsynth_run_batch(stack("style"), stack("source_guide"), stack("target_guide"),
                                   style_weights=jobs[0]["style_weights"], guide_weights=jobs[0]["guide_weights"],
                                   uniformity=cfg["uniformity"], patch_size=cfg["patchsize"],
                                   pyramid_levels=cfg["pyramidlevels"], search_vote_iters=cfg["searchvoteiters"],
                                   patchmatch_iters=cfg["patchmatchiters"], stop_threshold=cfg["stopthreshold"],
                                   extra_pass_3x3=cfg["extrapass3x3"], seeds=0)
    img, err = img.cpu().numpy(), err.cpu().numpy()
    return [(img[k], err[k]) for k in range(len(jobs))]


def write_output(output, img, err):
    """The shim's outputs: PNG content at `output` (whatever its extension), the error map at bin_path(output)."""
    from PIL import Image
    Image.fromarray(img[..., 0] if img.shape[2] == 1 else img).save(output, format="PNG")
    E.write_error_bin(E.bin_path(output), err)


def _guide_module(vb):
    """blender.guide as video_blend loaded it (its read_flow / read_mask), else flow.flow_utils."""
    for name in ("blender.guide", "flow.flow_utils"):
        m = sys.modules.get(name)
        if m is not None and hasattr(m, "read_flow") and hasattr(m, "read_mask"):
            return m
    raise RuntimeError("fresco_amd.propagate: load video_blend.py first (blender.guide is not imported)")


def run_ebsynth(vb, video_sequence, *, max_batch=None, synth=None, threads=8, stats=None):
    """video_blend.run_ebsynth(video_sequence) in this process (module docstring).  ``vb`` is the loaded video_blend
    module; ``synth(jobs) -> [(image, error)]`` replaces the batched GPU synthesis (tests); ``threads`` (<= 16) run the
    host work per chain; ``stats`` (a dict) receives the wall time per phase in seconds and the batch sizes."""
    cv2 = vb.cv2
    gm = _guide_module(vb)
    synth = gpu_synth if synth is None else synth
    dev = _device()
    st = stats if stats is not None else {}
    for k in ("flows", "guide_kernels", "host", "synthesis"):
        st[k] = 0.0
    st["batches"] = []
    beg = time.time()

    def timed(key, fn, *a):
        t0 = time.perf_counter()
        r = fn(*a)
        if key in ("guide_kernels", "synthesis"):
            torch.cuda.synchronize()
        st[key] += time.perf_counter() - t0
        return r

    chains = [Chain(video_sequence, i, fwd) for i in range(video_sequence.n_seq) for fwd in (True, False)]
    pool = ThreadPoolExecutor(max_workers=max(1, min(int(threads), MAX_THREADS)))
    try:
        # flows, exactly as process_one_sequence computes them; a batched flow_calc (fresco_amd.flowcalc.FlowCalc) takes
        # every chain's pairs in one call, each input frame read once
        def flows_of(c):
            for j in range(c.interval - 1):
                i1 = cv2.imread(c.inputs[j])
                i2 = cv2.imread(c.inputs[j + 1])
                vb.flow_calc.get_flow(i1, i2, c.flows[j])

        def batched_flows():
            paths, slot, pairs, saves = [], {}, [], []
            for c in chains:
                for j in range(c.interval - 1):
                    for p in c.inputs[j:j + 2]:
                        if p not in slot:
                            slot[p] = len(paths)
                            paths.append(p)
                    pairs.append((slot[c.inputs[j]], slot[c.inputs[j + 1]]))
                    saves.append(c.flows[j])
            if pairs:
                vb.flow_calc.get_flows(list(pool.map(cv2.imread, paths)), pairs, saves, return_flows=False)

        if hasattr(vb.flow_calc, "get_flows"):
            timed("flows", batched_flows)
        else:
            timed("flows", lambda: [flows_of(c) for c in chains])

        def read_chain(c):
            c.flow = [gm.read_flow(f) for f in c.flows]
            c.mask = [gm.read_mask(f) for f in c.flows]
            c.frames = [cv2.imread(p) for p in c.inputs]
            return c

        timed("host", lambda: list(pool.map(read_chain, chains)))

        # edge guides: every chain's input frames in one launch
        def edges():
            frames = torch.from_numpy(np.stack([f for c in chains for f in c.frames])).to(dev)
            return E.edge_guide(frames).cpu().numpy()

        edge = timed("guide_kernels", edges) if chains else []

        def write_static(k):
            c = chains[k]
            off = sum(len(x.frames) for x in chains[:k])
            for p, img in zip(c.edges, edge[off:off + len(c.frames)]):
                cv2.imwrite(p, img)
            cv2.imwrite(c.temporal[0], cv2.imread(c.key_img))  # TemporalGuide.__init__
            h, w = c.flow[0].shape[2:] if c.flow else c.frames[0].shape[:2]
            c.pos_imgs = [first_positional_image(h, w)]

        timed("host", lambda: list(pool.map(write_static, range(len(chains)))))

        # positional guides: warp (GPU, all chains at step k in one launch) then inpaint (host), chain by chain
        for k in range(max((len(c.flow) for c in chains), default=0)):
            live = [c for c in chains if len(c.flow) > k]

            def warp_pos():
                imgs = torch.from_numpy(np.stack([c.pos_imgs[k].astype(np.uint8) for c in live])).to(dev)
                fl = torch.cat([c.flow[k].reshape(1, 2, *c.flow[k].shape[-2:]) for c in live]).to(dev, torch.float32)
                return E.warp_nearest(imgs, fl).cpu().numpy()

            warped = timed("guide_kernels", warp_pos)

            def inpaint_pos(a):
                c, img = a
                c.pos_imgs.append(cv2.inpaint(img, c.mask[k], 30, cv2.INPAINT_TELEA))

            timed("host", lambda: list(pool.map(inpaint_pos, zip(live, warped))))

        def finish_static(c):
            for p, img in zip(c.pos, c.pos_imgs):
                cv2.imwrite(p, img)
            cv2.imwrite(c.outputs[0], cv2.imread(c.key_img))  # j == 0: the key frame
            c.cache = {}
            for path in [os.path.abspath(c.key_img)] + [os.path.abspath(s[0]) for s in
                                                        (c.inputs, c.edges, c.temporal, c.pos)]:
                c.cache[path] = E._load_rgba(path)
            return c

        timed("host", lambda: list(pool.map(finish_static, chains)))

        for j, live_idx in steps(chains):
            live = [chains[k] for k in live_idx]

            def read_prev(c):
                return cv2.imread(c.outputs[j - 1])

            prevs = timed("host", lambda: list(pool.map(read_prev, live)))

            def warp_prev():
                imgs = torch.from_numpy(np.stack(prevs)).to(dev)
                fl = torch.cat([c.flow[j - 1].reshape(1, 2, *c.flow[j - 1].shape[-2:]) for c in live])
                return E.warp_nearest(imgs, fl.to(dev, torch.float32)).cpu().numpy()

            warped = timed("guide_kernels", warp_prev)

            def temporal_and_load(a):
                c, img = a
                cv2.imwrite(c.temporal[j], cv2.inpaint(img, c.mask[j - 1], 30, cv2.INPAINT_TELEA))
                return load_job(c.argv(j), c.cache)

            jobs = timed("host", lambda: list(pool.map(temporal_and_load, zip(live, warped))))
            results = [None] * len(jobs)
            for b in batches(jobs, max_batch):
                st["batches"].append(len(b))
                for k, r in zip(b, timed("synthesis", synth, [jobs[k] for k in b])):
                    results[k] = r

            def write(a):
                c, (img, err) = a
                write_output(c.outputs[j], img, err)

            timed("host", lambda: list(pool.map(write, zip(live, results))))
    finally:
        pool.shutdown()
    end = time.time()
    print(f'ebsynth: {end-beg}')


def patch_run_ebsynth(vb, **kw):
    """Rebind ``vb.run_ebsynth`` (vb: the reference's loaded video_blend module) to ``run_ebsynth`` here; keyword
    arguments (max_batch, synth, threads, stats) are passed on.  Returns vb."""

    def run_ebsynth_(video_sequence):
        return run_ebsynth(vb, video_sequence, **kw)

    vb.run_ebsynth = run_ebsynth_
    return vb


__all__ = ["patch_run_ebsynth", "run_ebsynth", "compose_cmd", "compose_argv", "steps", "batches", "group_key",
           "load_job", "gpu_synth", "write_output", "first_positional_image", "Chain"]
