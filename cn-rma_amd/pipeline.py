"""The hot path end to end for one scene (SURVEY.md 8d metric):

    features [V,C,H,W] + projections [V,3,4] + TSDF [X,Y,Z]
      -> dense unprojection-accumulate (a1-a3)  -> volume, count          (input of the Atlas 3D CNN, out of scope)
      -> ray-marching aggregation (a4-a7) fused with the point selection (a8)
      -> voxelisation (a9) -> FCAF3D backbone (a10) -> neck + head (a11) -> decode (a12) -> raw boxes + scores

Mirrors the order of RayMarching.forward_test (projects/mvsdetection/models/ray_marching.py:456-521) with the 2D
backbone and the Atlas reconstruction network replaced by their outputs (features, TSDF) as inputs.
"""
import torch

from . import _lib, rma
from . import plan as P
from . import sparse as S


DEFER_POINT_FEATURES = True     # static trace: point features are emitted once, in voxel order, into the sparse tensor (trace_net)
DENSE_BRANCH = False     # StaticScene: the dense unprojection as a parallel branch of the scene graph (fork / join inside the
                         # capture).  Measured (bench.py --dense-branch 1): NS 40.8 vs 43.0 scenes/s, S 163 vs 202 -- a graph with a
                         # second stream in it replays slower than the linear chain, and the chip-filling kernel gains nothing


class SceneConfig:
    def __init__(self, dims, voxel_size=0.04, origin=(0.0, 0.0, 0.0), stride=4, n_steps=300, thr=0.05,
                 max_points=500000, voxel_size_fcaf3d=0.01, ray_marching_type="neus", depth_points=None,
                 sampler="device", sample_seed=None):
        self.dims = tuple(dims)
        self.voxel_size = voxel_size
        self.origin = tuple(origin)
        self.stride = stride
        self.n_steps = n_steps
        self.thr = thr
        self.max_points = max_points
        self.voxel_size_fcaf3d = voxel_size_fcaf3d
        self.ray_marching_type = ray_marching_type
        self.depth_points = depth_points
        self.sampler = sampler
        self.sample_seed = sample_seed        # device sampler: fixed seed (None = a fresh subset per call)


def graph_node_count(graph):
    """number of nodes of a captured torch.cuda.CUDAGraph (hipGraphGetNodes on its raw handle; the graph must have been
    created with keep_graph=True); None when the runtime does not give it"""
    import ctypes
    import os
    try:
        hip = ctypes.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
        n = ctypes.c_size_t(0)
        hip.hipGraphGetNodes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
        hip.hipGraphGetNodes.restype = ctypes.c_int
        if hip.hipGraphGetNodes(ctypes.c_void_p(graph.raw_cuda_graph()), None, ctypes.byref(n)) != 0:
            return None
        return int(n.value)
    except Exception:       # noqa: BLE001 -- a diagnostic: never fatal
        return None


def weight_tensors(*modules):
    """every parameter and buffer of the modules, as a list (built once per captured context)"""
    import itertools
    return [t for m in modules for t in itertools.chain(m.parameters(), m.buffers())]


def weights_tag(tensors):
    """cheap fingerprint of a model's weights: (count, sum of in-place version counters, first storage address).  Optimiser
    steps, load_state_dict() and every other in-place write bump a version; a moved / re-created model changes the
    address.  (Writes through `.data` bump nothing: call the owner's reset after those.)  A captured graph replays
    prepared weight images, so its owner compares this tag before each replay."""
    v = 0
    for t in tensors:
        v += t._version
    return (len(tensors), v, tensors[0].data_ptr() if tensors else 0)


def _offset_list(offset):
    if offset is None:
        return (0.0, 0.0, 0.0)
    return tuple(float(x) for x in torch.as_tensor(offset, dtype=torch.float32).detach().reshape(3).cpu().tolist())


class StageTimer:
    """optional per-stage HIP-event timing on the current stream"""

    def __init__(self, enabled):
        self.enabled = enabled
        self.marks = []

    def mark(self, name):
        if self.enabled:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self.marks.append((name, e))

    def result(self):
        if not self.enabled:
            return {}
        torch.cuda.synchronize()
        out = {}
        for (_, a), (n, b) in zip(self.marks[:-1], self.marks[1:]):
            out[n] = out.get(n, 0.0) + a.elapsed_time(b)
        return out


@torch.no_grad()
def forward_scenes(cfg, backbone, head, scenes):
    """Several scenes through ONE sparse network pass.  scenes: list of dicts(features [V,C,H,W], projection [V,3,4],
    tsdf [X,Y,Z], offset=(0,0,0)).  The geometric half (dense unprojection, ray marching, selection, voxelisation)
    runs per scene; the scenes' voxels are then collated into one multi-scene sparse tensor (batch id = list index,
    ray_marching.py:328-330 builds exactly that for B samples) for the backbone + neck/head, whose ~300 small launches
    and split-K tails are thereby shared; decode is per scene.  Returns one dict per scene like forward_scene()."""
    parts, infos, states = [], [], []
    for sc_ in scenes:                                   # phase 1: everything up to the row-count read-back, all scenes
        feats = rma.to_nhwc(sc_["features"])
        volume, count = rma.backproject_accum(feats, sc_["projection"], cfg.dims, cfg.voxel_size, cfg.origin, cfg.stride)
        proj_inv = rma.projection_inverse(sc_["projection"], cfg.stride).to(feats.device, non_blocking=True)
        states.append(rma.aggregate_begin(feats, proj_inv, sc_["tsdf"], cfg.dims, cfg.voxel_size, cfg.origin, cfg.n_steps,
                                          cfg.thr, cfg.ray_marching_type, cfg.depth_points))
        infos.append(dict(volume=volume, count=count))
    reads = _lib.read_ints(torch.cat([st["readback"] for st in states]))       # ONE device->host read for all scenes
    w = len(reads) // len(scenes)
    for b, (sc_, st) in enumerate(zip(scenes, states)):    # phase 2: selection + emission
        coords, pfeats, info = rma.aggregate_finish(st, reads[b * w:(b + 1) * w], sc_.get("offset", (0.0, 0.0, 0.0)),
                                                    cfg.max_points, cfg.sampler, sc_.get("mask"))
        parts.append((coords, pfeats))
        infos[b].update(info)
    x = S.sparse_collate(parts, cfg.voxel_size_fcaf3d)
    levels = backbone(x)
    cen, box, cls, pts, scn = map(list, head(levels, fused=True))
    dets = head.get_bboxes_fused(cen, box, cls, pts, scn, len(scenes))
    outs = []
    for b, (bboxes, scores) in enumerate(dets):
        outs.append(dict(bboxes=bboxes, scores=scores, M=infos[b]["M"], M_selected=infos[b]["M_selected"],
                         M_unique=x.cs.batch_counts()[b], volume=infos[b]["volume"], count=infos[b]["count"],
                         level_rows=[len(l) for l in levels], head_rows=[len(c[0]) for c in cen]))
    return outs


@torch.no_grad()
def forward_scene(cfg, backbone, head, features_nchw, projections, tsdf, offset=(0.0, 0.0, 0.0), dense=True,
                  timing=False, mask=None, proj_inv=None, keep_half=False):
    """One scene forward.  features_nchw [V,C,H,W] device fp32 (the 2D backbone's layout), projections [V,3,4]
    (full-resolution pixel units; a host copy avoids a D2H), tsdf [X,Y,Z] device.  Returns a dict with the decoded
    boxes/scores and the intermediate sizes needed to recompute the algorithmic bytes.
    keep_half: fp16 / bf16 maps stay 16-bit and the dense unprojection and the NeuS row emission read them in place (same
    results, bit for bit, as on the maps widened to fp32 -- which is what happens by default); depth mode widens them."""
    tm = StageTimer(timing)
    tm.mark("start")
    feats = rma.to_nhwc(features_nchw, keep_dtype=keep_half)
    tm.mark("nhwc")
    out = {}
    if dense:
        volume, count = rma.backproject_accum(feats, projections, cfg.dims, cfg.voxel_size, cfg.origin, cfg.stride)
        out["volume"], out["count"] = volume, count
        tm.mark("dense")
    if proj_inv is None:
        proj_inv = rma.projection_inverse(projections, cfg.stride)
    proj_inv = proj_inv.to(feats.device, non_blocking=True)
    coords, pfeats, info = rma.aggregate_points(
        feats, proj_inv, tsdf, cfg.dims, cfg.voxel_size, cfg.origin, cfg.n_steps, cfg.thr, cfg.ray_marching_type,
        cfg.depth_points, offset=offset, max_points=cfg.max_points, sampler=cfg.sampler, mask=mask, seed=cfg.sample_seed)
    tm.mark("rma")
    x, _ = S.voxelize(coords, pfeats, cfg.voxel_size_fcaf3d)
    if P.current() is not None:
        P.current().mark("net")              # what follows scales with the number of scenes in a pass (Plan.scaled)
    tm.mark("voxelize")
    levels = backbone(x)
    tm.mark("backbone")
    cen, box, cls, pts = map(list, head(levels))
    tm.mark("head")
    bboxes, scores = head.get_bboxes_scene(cen, box, cls, pts)
    tm.mark("decode")
    out.update(bboxes=bboxes, scores=scores, M=info["M"], M_selected=info["M_selected"], M_unique=len(x),
               level_rows=[len(l) for l in levels], head_rows=[len(c[0]) for c in cen], stage_ms=tm.result())
    return out


def trace_nms(plan, out, nms, state, nms_pre=0):
    """the opt-in last stage of a static trace: per-class NMS of the padded detections on the device (postprocess.nms_device,
    four launches on the same stream: the captured sequence stays a linear chain).  nms = dict(score_thr=..., iou_thr=...);
    `state` belongs to the traced object and holds the workspace and the outputs, allocated by its first static run and pinned
    for the life of the plan.  Adds nms_boxes / nms_scores / nms_labels (capacity-sized) and nms_n (device int32 [1]).
    A level that keeps all its rows owns its whole capacity in the block, but the plan holds it to nms_pre live rows (more
    is a violation: status != 0): such segments are cut to nms_pre rows first (two copies more), so that four levels of
    nms_pre <= 1024 always fit the kernel's 4096 rows."""
    from . import postprocess
    b, sc, sizes = out["bboxes"], out["scores"], list(out["sizes"])
    if nms_pre > 0 and any(k > nms_pre for k in sizes):
        starts = [sum(sizes[:l]) for l in range(len(sizes))]
        sizes = [min(k, nms_pre) for k in sizes]
        b = torch.cat([b[r0:r0 + k] for r0, k in zip(starts, sizes)])
        sc = torch.cat([sc[r0:r0 + k] for r0, k in zip(starts, sizes)])
    if b.shape[0] > postprocess.NMS_DEVICE_MAX_ROWS:
        raise _lib.CnrmaError(f"nms= needs a detection block of at most {postprocess.NMS_DEVICE_MAX_ROWS} rows, the plan's "
                              f"levels {sizes} add up to {b.shape[0]}")
    key = (b.shape[0], sc.shape[1], b.shape[1], b.device)
    if state.get("key") != key:
        state.clear()
        state.update(key=key, bufs=postprocess.nms_device_buffers(b.shape[0], sc.shape[1], b.shape[1], b.device))
    bufs = state["bufs"]
    plan.keep(*bufs.values())
    boxes, scores, labels, n = postprocess.nms_device(b, sc, valid=out["valid"], sizes=sizes, padded=True, out=bufs, **nms)
    out.update(nms_boxes=boxes, nms_scores=scores, nms_labels=labels, nms_n=n)


def check_nms_setting(nms):
    if nms is not None and not (isinstance(nms, dict) and set(nms) <= {"score_thr", "iou_thr"}):
        raise ValueError(f"nms must be None or dict(score_thr=..., iou_thr=...), got {nms!r}")
    return None if nms is None else dict(nms)


def _read_back(out, extra=()):
    """the ONE device->host read of a static output, on the current stream once out["done"] has completed: the host values of
    `valid`, `counts` and the `extra` words, in that order.  Raises when the pass violated an assumption of its plan (status != 0)."""
    if out.get("done") is not None:
        torch.cuda.current_stream(out["bboxes"].device).wait_event(out["done"])
    host = _lib.read_ints(torch.cat([out[k].view(-1) for k in ("status", "valid", "counts", *extra)]))
    if host[0] != 0:
        raise _lib.CnrmaError(f"{host[0]} capacity / branch assumption(s) of the static plan violated: re-run eagerly")
    return host[1:]


def _live_rows(sizes, valid, device):
    """index of the detections in a padded block: level l owns rows [sum(sizes[:l]), +sizes[l]), the first valid[l] are live"""
    rows, r0 = [], 0
    for k, v in zip(sizes, valid):
        rows.append(torch.arange(r0, r0 + v, device=device))
        r0 += k
    return torch.cat(rows)


def final_detections(out):
    """(boxes [K, 6|7], scores [K], labels [K]) of a static output traced with nms=...: what postprocess.nms makes of
    detections(out), after ONE device->host read (status, valid, counts and the detection count together)"""
    if "nms_n" not in out:
        raise _lib.CnrmaError("this static trace was built without nms=...: it ends at the raw detections")
    k = min(_read_back(out, ("nms_n",))[-1], out["nms_boxes"].shape[0])
    return out["nms_boxes"][:k], out["nms_scores"][:k], out["nms_labels"][:k]


def trace_net(plan, backbone, head, coords, feats, n_dev, voxel_size, device, extra_counts=(), late=None, nms=None,
              nms_state=None):
    """the sparse half inside a static trace (plan.static): voxelise -> MinkResNet34 -> neck / head -> decode of the point
    rows [0, n_dev) of the capacity-sized (coords, feats).  Returns the padded detections, the per-level head outputs and
    one small tensor of live counts -- no device->host read.
    nms (dict(score_thr, iou_thr), with the caller's nms_state): the per-class NMS is appended, see trace_nms.
    late (feats is None): the aggregation's info with the point RECORDS instead of features -- the voxeliser carries the
    16-byte records (as 4-float rows) through its representative selection and sort, and the features of the surviving rows
    are emitted straight into the sparse tensor, with their magnitude bound: no [M, C] intermediate, no row gather, no
    absmax pass (0.27 ms per scene at the north-star shape)."""
    if feats is None:
        rec_f = late["rec"].view(torch.float32)                        # bit patterns travel through float4 copies untouched
        xr, _ = S.voxelize(coords, rec_f, voxel_size, n_dev=n_dev)
        amax = S._amax_slot(device)
        F = rma.emit_point_features(late, xr.F.view(torch.int32), xr.cs.n, xr.cs.n_dev, amax=amax)
        x = S.SparseTensor(F, xr.cs, None, amax)
    else:
        x, _ = S.voxelize(coords, feats, voxel_size, n_dev=n_dev)
    levels = backbone(x)
    cen, box, cls, pts, css = map(list, head(levels, fused=True))
    bboxes, scores, valid, sizes = head.get_bboxes_static(cen, box, cls, pts, css)
    status = plan.status(device)
    # every live count of the pass in ONE small tensor (read together with the detections, if at all)
    counts = torch.cat([c.view(1) for c in extra_counts] + [x.cs.n_dev.view(1)] + [l.cs.n_dev.view(1) for l in levels] +
                       [c[0].n_dev.view(1) for c in css]).to(torch.int32)
    out = dict(bboxes=bboxes, scores=scores, valid=valid, sizes=sizes, status=status, counts=counts, n_levels=len(levels),
               n_extra=len(extra_counts), levels=levels,
               head=dict(centerness=[c[0] for c in cen], bbox_pred=[b[0] for b in box], cls_score=[c[0] for c in cls],
                         points=[p[0] for p in pts], n_dev=[c[0].n_dev for c in css]))
    if nms is not None:
        trace_nms(plan, out, nms, nms_state, head.nms_pre)
    return out


class _StaticGraph:
    """What StaticNet, StaticScene and StaticBatch share: a launch sequence (`_trace`, run under the object's size plan) on the
    object's own stream, traced once plainly and once under stream capture, then replayed per call on inputs that `_load`
    staged into static buffers.  Subclasses bring `_load`, `_trace` and what is theirs alone."""

    def __init__(self, device, margin, stream):
        self.device = torch.device(device)
        self.margin = margin
        self.stream = stream if stream is not None else torch.cuda.Stream(device=self.device)
        self.plan = self.graph = self.out = self.done = None

    def _enter(self, *tensors):
        """order self.stream behind the caller's stream (the 2D backbone / Atlas head that produced the inputs ran there) and
        keep the inputs' memory from being recycled while self.stream still reads it"""
        cur = torch.cuda.current_stream(self.device)
        if cur != self.stream:
            self.stream.wait_stream(cur)
            for t in tensors:
                if torch.is_tensor(t) and t.is_cuda:
                    t.record_stream(self.stream)

    def _capture(self, capture):
        """with the inputs loaded and self.stream current: the plain static run (it creates the trace's device constants and is
        what the tests compare with the eager result), then the same sequence under stream capture"""
        self.out = self._trace()
        self.stream.synchronize()
        if capture:
            self._record()
            self.stream.synchronize()

    def _record(self, graph=None):
        """the launch sequence under stream capture, into `graph` when a subclass brings its own"""
        self.graph = graph if graph is not None else torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=self.stream):
            self.out = self._trace()

    def _replay(self):
        """with the inputs loaded and self.stream current: one pass, and the event that tells its end"""
        if self.graph is not None:
            self.graph.replay()
        else:
            self.out = self._trace()
        self.done = torch.cuda.Event()
        self.done.record()
        self.out["done"] = self.done
        return self.out


class StaticNet(_StaticGraph):
    """The sparse half alone (point rows -> raw detections) as a replayable HIP graph: what StaticScene runs after the
    aggregation, without the geometric half in front.  Used to pin the graph path of the network to the oracle on
    arbitrary point sets (tests) and by callers that bring their own points."""

    def __init__(self, backbone, head, voxel_size, device, margin=1.2, stream=None, nms=None):
        """nms: None (the trace ends at the raw detections) or dict(score_thr=..., iou_thr=...): the per-class NMS runs on the
        device at the end of the trace (out["nms_boxes" / "nms_scores" / "nms_labels" / "nms_n"], final_detections())"""
        super().__init__(device, margin, stream)
        self.backbone, self.head, self.voxel_size = backbone, head, voxel_size
        self.nms, self._nms_state = check_nms_setting(nms), {}

    def build(self, coords, feats, capture=True, cap=None):
        """calibrate eagerly on (coords [M,3], feats [M,C]), then trace statically at point capacity `cap` (default M)
        and capture.  Returns the eager result dict(bboxes, scores)."""
        _lib.require_gpu()
        self._enter(coords, feats)
        with torch.cuda.stream(self.stream), torch.no_grad():
            plan = P.Plan(self.margin)
            with P.using(plan):
                x, _ = S.voxelize(coords, feats, self.voxel_size)
                levels = self.backbone(x)
                cen, box, cls, pts = map(list, self.head(levels))
                bboxes, scores = self.head.get_bboxes_scene(cen, box, cls, pts)
            self.plan = plan
            M, C = feats.shape
            self.cap = int(cap or M)
            self.coords = torch.zeros((self.cap, 3), dtype=torch.float32, device=self.device)
            self.feats = torch.zeros((self.cap, C), dtype=torch.float32, device=self.device)
            self.n_dev = torch.zeros(1, dtype=torch.int32, device=self.device)
            self._load(coords, feats)
            self._capture(capture)
        return dict(bboxes=bboxes, scores=scores, level_rows=[len(l) for l in levels])

    def _load(self, coords, feats):
        n = coords.shape[0]
        assert n <= self.cap
        self.coords[:n].copy_(coords, non_blocking=True)
        self.feats[:n].copy_(feats, non_blocking=True)
        self.n_dev.fill_(n)

    def _trace(self):
        self.plan.begin_static()
        with P.using(self.plan), torch.no_grad():
            out = trace_net(self.plan, self.backbone, self.head, self.coords, self.feats, self.n_dev, self.voxel_size,
                            self.device, nms=self.nms, nms_state=self._nms_state)
        self.plan.end_static()
        return out

    def run(self, coords, feats):
        self._enter(coords, feats)
        with torch.cuda.stream(self.stream):
            self._load(coords, feats)
            return self._replay()

    final_detections = staticmethod(final_detections)


class StaticScene(_StaticGraph):
    """One scene forward as a replayable HIP graph: the whole launch sequence of forward_scene() (dense unprojection,
    march, selection, voxelisation, MinkResNet34, neck/head, decode -- ~350 launches) captured once and replayed per
    scene with a single host call; no device->host read, no allocation, no Python in between.

    build() runs the scene eagerly once under a recording plan.Plan (every data-dependent row count is read back, as
    the reference does at nonzero() / in ME's coordinate manager), derives capacities (recorded size x `margin`) and
    re-runs the sequence in static mode -- once plainly (this creates the trace's device constants and is compared with
    the eager result by the tests), once under stream capture.  run() then costs: one layout kernel (the 2D backbone's
    NCHW maps -> the static channels-last buffer), three small input copies, one graph launch.  The outputs are static
    buffers, valid until the next run() of this object; `status` (device int32) counts violated capacity / branch
    assumptions -- non-zero means the scene outgrew the plan and must be re-run eagerly (forward_scene)."""

    def __init__(self, cfg, backbone, head, device, margin=1.2, dense=True, stream=None, by_reference=True,
                 feature_dtype=torch.float32, nms=None):
        """nms: None (default: the graph ends at the raw detections, exactly as without the argument) or
        dict(score_thr=..., iou_thr=...): the per-class NMS of postprocess.nms is appended to the captured sequence (four launches,
        same stream) and final_detections(out) returns boxes, scores and labels after the scene's one device->host read.
        feature_dtype: the ONE element type of this slot's feature maps.  torch.float32 (default): maps of any dtype are
        converted, as ever.  torch.float16 / torch.bfloat16 (NeuS mode, C % 8 == 0): the trace reads 16-bit maps -- in place when
        they are channels-last in memory, through the 16-bit layout pass into a buffer of half the size otherwise -- and run()
        with maps of another dtype raises ValueError (rounding fp32 maps to 16 bits silently is not a hand-off)."""
        self.cfg, self.backbone, self.head = cfg, backbone, head
        self.nms, self._nms_state = check_nms_setting(nms), {}
        self.feature_dtype = feature_dtype
        if feature_dtype != torch.float32:
            if feature_dtype not in rma.ELEM_CODES:
                raise ValueError(f"feature_dtype must be torch.float32, torch.float16 or torch.bfloat16, got {feature_dtype}")
            if cfg.ray_marching_type != "neus":
                raise ValueError("16-bit feature maps are read by the NeuS path only: depth mode takes a float32 slot")
        super().__init__(device, margin, stream)
        self.dense = dense
        # feature hand-off of channels-last maps (run()'s `by_reference` overrides it per scene): True = the trace reads the
        # caller's tensor in place for the WHOLE replay; False = copied into the slot's own buffer first
        self.by_reference = bool(by_reference)
        self._copied = self._held = None
        self.nhwc = self.march = self.march_out = self.seed_dev = None      # static input buffers: _alloc_inputs (build)
        self._dense_ws = self._side = None     # the dense kernel's workspace and DENSE_BRANCH's stream, made on first use
        self.n_nodes = None                # launches per scene of the captured graph (bench: graph_nodes_per_scene)
        self.arena_fallbacks = 0
        self.outgrown, self.n_outgrown = None, 0      # sizes of the scenes that outgrew the plan since the last (re)build
        self.check_weights = True          # compare the weights' fingerprint before every replay (~20 us of host time)
        self._weights = weight_tensors(backbone, head)
        self._tag = None

    # ---- inputs --------------------------------------------------------------------------------------------------
    def _alloc_inputs(self, features_nchw, tsdf):
        V, C, H, W = features_nchw.shape
        dev = self.device
        if self.feature_dtype != torch.float32 and C % 8 != 0:
            raise ValueError(f"a {self.feature_dtype} slot needs C % 8 == 0 (one 16-byte load is 8 channels), got C = {C}")
        self.shape_nhwc = (V, H, W, C)
        # The kernels of the trace read the feature maps BY REFERENCE (feat_ref: a device word with their address, written per
        # scene): maps that are channels-last in memory -- what the 2D network hands over when it runs in
        # torch.channels_last -- are read where they lie; NCHW maps go through the layout pass into `nhwc`, a buffer that is
        # only allocated when the first such scene arrives (12.6 GB at the north-star shape).
        self.nhwc = None
        self.feat_ref = torch.zeros(1, dtype=torch.int64, device=dev)
        self._pin_ref = torch.zeros(1, dtype=torch.int64, pin_memory=True)
        self._held = None
        self.proj_scaled = torch.empty((V, 3, 4), dtype=torch.float32, device=dev)
        self.proj_inv = torch.empty((V, 4, 4), dtype=torch.float32, device=dev)
        self.tsdf = torch.empty(tuple(self.cfg.dims), dtype=torch.float32, device=dev)
        self.seed_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        self.offset_dev = torch.zeros(3, dtype=torch.float32, device=dev)       # switch_pointcloud's per-scene offset
        self._pin_off = torch.zeros(3, dtype=torch.float32, pin_memory=True)
        cfg = self.cfg
        # the march runs with the layout pass, in _load (one launch), into buffers the graph reads
        self.march = self.march_out = None
        if cfg.ray_marching_type == "neus":
            self.march = rma._March(None, self.proj_inv, self.tsdf, cfg.dims, cfg.voxel_size, cfg.origin, cfg.n_steps,
                                    cfg.thr, "neus", 0, shape=self.shape_nhwc, device=dev, feat_ref=self.feat_ref,
                                    feat_dtype=self.feature_dtype)
            if self.march.kept_cap() <= 0:
                raise _lib.CnrmaError("the static trace needs the single-march NeuS path (thr > 1/62)")
            self.march_out = self.march.march_buffers()
        else:
            self._nhwc_buffer()                  # depth mode: its emission kernel reads the static channels-last copy
        self._pin_proj = torch.empty((V, 3, 4), dtype=torch.float32, pin_memory=True)
        self._pin_inv = torch.empty((V, 4, 4), dtype=torch.float32, pin_memory=True)

    def _nhwc_buffer(self):
        """the slot's own channels-last feature buffer [V,H,W,C] (layout-pass target for NCHW inputs; producers may also write
        their output straight into it and call run(None, ...))"""
        if self.nhwc is None:
            self.nhwc = torch.empty(self.shape_nhwc, dtype=self.feature_dtype, device=self.device)
            if self.march is not None:
                self.march.feat = self.nhwc
        return self.nhwc

    def _load(self, features_nchw, projections, tsdf, proj_inv=None, offset=None, by_reference=None):
        """stage one scene's inputs into the static buffers (on self.stream, which must be current).  by_reference: see
        run().  proj_inv: the
        [V,4,4] inverse of [P/stride; 0 0 0 1] when the caller pins it (parity tests: LAPACK's inverse is not bit-stable
        across host CPUs); computed here on the host like ray_marching.py:96-102 otherwise."""
        if features_nchw is not None and self.feature_dtype != torch.float32 and features_nchw.dtype != self.feature_dtype:
            raise ValueError(f"this slot reads {self.feature_dtype} feature maps, got {features_nchw.dtype}: convert them "
                             "explicitly or use a slot of their dtype")
        if self._copied is not None:
            self._copied.synchronize()           # the previous scene's copies out of the pinned buffers have executed
        p = projections.detach().to("cpu", torch.float32)
        self._pin_proj.copy_(rma.scale_projection(p, self.cfg.stride))
        self._pin_inv.copy_(rma.projection_inverse(p, self.cfg.stride) if proj_inv is None
                            else proj_inv.detach().to("cpu", torch.float32))
        self.proj_scaled.copy_(self._pin_proj, non_blocking=True)
        self.proj_inv.copy_(self._pin_inv, non_blocking=True)
        self.tsdf.copy_(tsdf.reshape(self.tsdf.shape), non_blocking=True)
        if offset is None:
            self._pin_off.zero_()
        else:
            self._pin_off.copy_(torch.as_tensor(offset, dtype=torch.float32).detach().reshape(3).cpu())
        self.offset_dev.copy_(self._pin_off, non_blocking=True)
        # where the trace reads the feature maps from: features_nchw None = the caller already wrote _nhwc_buffer(); maps that
        # are channels-last in memory are read in place (NeuS mode); everything else goes through the layout pass (NCHW ->
        # the slot's buffer, in ONE launch with the march)
        layout_from = None
        by_reference = self.by_reference if by_reference is None else bool(by_reference)
        self._held = None
        in_place = rma.is_channels_last(features_nchw, (self.feature_dtype,))
        if in_place and self.feature_dtype != torch.float32 and features_nchw.data_ptr() % 16 != 0:
            by_reference = False                 # the 16-bit kernels load 16 bytes at a time: a misaligned view is copied
        if features_nchw is None:
            addr = self._nhwc_buffer().data_ptr()
        elif in_place and self.march is not None and by_reference:
            assert tuple(features_nchw.shape) == (self.shape_nhwc[0], self.shape_nhwc[3], self.shape_nhwc[1], self.shape_nhwc[2])
            addr = features_nchw.data_ptr()
            self._held = features_nchw           # alive until this slot takes its next scene
        elif in_place:
            self._nhwc_buffer().copy_(features_nchw.permute(0, 2, 3, 1), non_blocking=True)
            addr = self.nhwc.data_ptr()
        else:
            addr = self._nhwc_buffer().data_ptr()
            layout_from = features_nchw
        self._pin_ref[0] = addr
        self.feat_ref.copy_(self._pin_ref, non_blocking=True)
        self._copied = torch.cuda.Event()
        self._copied.record()                    # the pinned staging buffers are free again once this point has executed
        if self.march is not None:
            self.march.march(layout_from=layout_from, into=self.march_out)
        elif layout_from is not None:            # depth mode: the layout pass alone (its two small kernels run inside the trace)
            rma.to_nhwc(layout_from, out=self.nhwc)
        self._consumed = torch.cuda.Event()      # copies and the layout pass are behind this point: unless the maps are read
        self._consumed.record()                  # by reference (self._held), the caller's feature tensor is free again

    def _dense_workspace(self):
        """this scene's own workspace of the dense kernel (arrival counters + view masks): the captured graph replays into it, so
        it lives as long as the scene"""
        if self._dense_ws is None:
            self._dense_ws = rma.dense_workspace(self.device, self.cfg.dims, self.shape_nhwc[0], self.shape_nhwc[3],
                                                 self.feature_dtype in rma.ELEM_CODES)
        return self._dense_ws

    # ---- the launch sequence ---------------------------------------------------------------------------------------
    def _geometry(self, seed=0x5EED, defer_feats=False, side=None):
        """the geometric half of a static trace on the inputs this scene has loaded: the dense unprojection (self.dense; on the
        stream `side` when given) and the aggregation with its point selection, drawn with cfg.sample_seed when that is fixed
        (every replay draws the same subset, as forward_scene) and with `seed` + the scene's device counter otherwise.
        Returns ((volume, count) or None, coords, feats, n_sel, info); stepping seed_dev is left to the caller's sequence."""
        cfg = self.cfg
        dense = None
        if self.dense:
            with torch.cuda.stream(side if side is not None else torch.cuda.current_stream(self.device)):
                dense = rma.backproject_accum(None, None, cfg.dims, cfg.voxel_size, cfg.origin, cfg.stride,
                                              proj_scaled=self.proj_scaled, feat_ref=self.feat_ref, shape=self.shape_nhwc,
                                              feat_dtype=self.feature_dtype, workspace=self._dense_workspace())
        fixed = cfg.sample_seed is not None
        return (dense,) + rma.aggregate_points_static(
            self.nhwc, self.proj_inv, self.tsdf, cfg.dims, cfg.voxel_size, cfg.origin, cfg.n_steps, cfg.thr,
            max_points=cfg.max_points, seed=cfg.sample_seed if fixed else seed, seed_dev=None if fixed else self.seed_dev,
            marched=(self.march, self.march_out) if self.march is not None else None,
            mode=cfg.ray_marching_type, select_grids=cfg.depth_points or 0, feat_ref=self.feat_ref, shape=self.shape_nhwc,
            defer_feats=defer_feats, feat_dtype=self.feature_dtype)

    def _trace(self):
        cfg, plan = self.cfg, self.plan
        plan.begin_static()
        out = {}
        with P.using(plan), torch.no_grad():
            side = None
            if self.dense and DENSE_BRANCH:
                # the dense volume is an output of the scene (the Atlas 3D network's input), nothing downstream in the hot path
                # reads it: DENSE_BRANCH runs it as a parallel branch of the graph (forked stream, joined at the end) -- off
                # by default, see the note at the switch
                if self._side is None:
                    self._side = torch.cuda.Stream(device=self.device)
                side = self._side
                side.wait_stream(torch.cuda.current_stream(self.device))
            dense, coords, feats, n_sel, info = self._geometry(defer_feats=DEFER_POINT_FEATURES, side=side)
            if dense is not None:
                out["volume"], out["count"] = dense
            moved = coords + self.offset_dev     # ray_marching.py:364 (one fp32 add per coordinate, as the reference)
            out.update(trace_net(plan, self.backbone, self.head, moved, feats, n_sel, cfg.voxel_size_fcaf3d, self.device,
                                 extra_counts=[info["M"], n_sel], late=info, nms=self.nms, nms_state=self._nms_state))
            if cfg.sample_seed is None:
                self.seed_dev.add_(1)            # the next replay draws a fresh point subset
            if side is not None:
                torch.cuda.current_stream(self.device).wait_stream(side)          # join
        plan.end_static()
        # the aggregated points: places and row count are static outputs; with deferred features the [cap, C] rows are
        # produced on demand from the slot's records (point_features(): one launch outside the graph, on the caller's stream)
        out.update(points=(coords, feats, n_sel), points_info=info if feats is None else None)
        return out

    @staticmethod
    def point_features(out):
        """features [cap, C] of the aggregated points of a static output (rows >= out["points"][2] undefined): the stored rows,
        or -- deferred emission -- emitted now from the slot's records (valid until the slot's next run)"""
        coords, feats, n_sel = out["points"]
        if feats is None:
            if out.get("done") is not None:
                torch.cuda.current_stream(coords.device).wait_event(out["done"])
            feats = rma.point_features(out["points_info"])
        return feats

    def calibrate(self, features_nchw, projections, tsdf, proj_inv=None, offset=None):
        """one eager forward under a recording plan; several calls (several scenes of the configuration) are merged:
        capacities then cover the largest of them.  Returns the eager result."""
        _lib.require_gpu()
        self._enter(features_nchw, tsdf)
        with torch.cuda.stream(self.stream):
            plan = P.Plan(self.margin)
            with P.using(plan):
                eager = forward_scene(self.cfg, self.backbone, self.head, features_nchw, projections, tsdf, dense=self.dense,
                                      proj_inv=proj_inv, offset=_offset_list(offset),
                                      keep_half=self.feature_dtype != torch.float32)
        self.plan = plan if self.plan is None else self.plan.merge(plan)
        return eager

    def build(self, features_nchw, projections, tsdf, capture=True, plan=None, proj_inv=None):
        """calibrate on this scene (eager) unless calibrate() has been called or a finished `plan` of the same
        configuration is handed in (its sizes/flags are copied), then trace statically and capture.
        Returns the eager result of the calibration done here (None otherwise)."""
        _lib.require_gpu()
        eager = None
        if plan is not None:
            self.plan = plan.copy()
        elif self.plan is None:
            eager = self.calibrate(features_nchw, projections, tsdf, proj_inv)
        self._enter(features_nchw, tsdf)
        with torch.cuda.stream(self.stream):
            self._alloc_inputs(features_nchw, tsdf)
            self._load(features_nchw, projections, tsdf, proj_inv)
            self._capture(capture)
        self._tag = weights_tag(self._weights)
        return eager

    def _record(self):
        try:                                                 # keep_graph only serves the node count, a diagnostic
            kept = torch.cuda.CUDAGraph(keep_graph=True)
        except TypeError:                                    # a torch build without it: capture instantiates by itself
            kept = None
        super()._record(kept)
        kept = kept is not None
        self.n_nodes = graph_node_count(self.graph) if kept else None
        # tables of the CAPTURED trace that did not fit the 0xFF arena its sizing run measured (each clears itself: one
        # launch more; 0 unless the two runs took different table sequences -- ADVICE round 5)
        self.arena_fallbacks = self.plan.arena_fallbacks
        if kept:
            self.graph.instantiate()

    def run(self, features_nchw, projections, tsdf, proj_inv=None, offset=None, by_reference=None):
        """enqueue one scene on self.stream (ordered behind the caller's current stream, which produced the inputs);
        returns the static output dict (device tensors, valid until the next run; consumers on another stream wait on
        `self.done` first -- detections() does).

        Feature hand-off (`by_reference`, None = the slot's default set at construction, True unless told otherwise):
        * maps that are channels-last in memory and by_reference=True: the captured graph reads the CALLER'S tensor in
          place during the whole replay (~16 ms at the north-star shape, with up to `slots` scenes in flight).  CONTRACT: the
          caller must not write that memory -- no in-place op, no reuse of a preallocated / double-buffered / graph-static
          output buffer of the 2D network -- until `out["done"]` has completed.  The slot only keeps the memory from being
          freed or recycled (it holds the tensor and record_stream()s it); an in-place overwrite corrupts the dense volume
          and the point features silently (the plan status stays 0).
        * by_reference=False (or NCHW maps, always): the maps are copied / converted into the slot's own buffer (12.6 GB
          at the north-star shape, allocated on first use) before the trace starts; the caller may overwrite them as soon
          as `out["inputs_consumed"]` (an event on the slot's stream) has completed."""
        if self.graph is not None and self.check_weights and weights_tag(self._weights) != self._tag:
            raise _lib.CnrmaError("the model's weights changed since this scene graph was captured (optimiser step, "
                                  "load_state_dict, .to()): the graph replays prepared weight images -- rebuild() it")
        self._enter(features_nchw, tsdf)
        with torch.cuda.stream(self.stream):
            self._load(features_nchw, projections, tsdf, proj_inv, offset, by_reference)
            consumed = self._consumed
            self._replay()
        # when the caller may write the feature maps again: by reference -> only after the whole scene
        self.out["inputs_consumed"] = self.done if self._held is not None else consumed
        return self.out

    def rebuild(self, features_nchw, projections, tsdf):
        """fold the sizes of the scenes that outgrew the plan (the eager fall-backs) into the plan and trace / capture
        again at the larger capacities"""
        if self.outgrown is not None:
            self.plan.static = False
            self.plan = self.plan.merge(self.outgrown) if len(self.plan.sizes) == len(self.outgrown.sizes) else self.outgrown
            self.outgrown, self.n_outgrown = None, 0
        return self.build(features_nchw, projections, tsdf, capture=True, plan=self.plan)

    @staticmethod
    def detections(out):
        """static outputs -> (bboxes [K,*], scores [K,n_cls], info) like forward_scene; ONE device->host read.  Raises
        when the scene violated an assumption of the plan (the caller re-runs it with forward_scene)."""
        L = len(out["sizes"])
        host = _read_back(out)
        valid, counts = host[:L], host[L:]
        rows = _live_rows(out["sizes"], valid, out["bboxes"].device)
        nl, ne = out["n_levels"], out.get("n_extra", 2)
        info = dict(M_unique=counts[ne], level_rows=counts[ne + 1:ne + 1 + nl], head_rows=counts[ne + 1 + nl:ne + 1 + 2 * nl])
        if ne == 2:
            info.update(M=counts[0], M_selected=counts[1])
        return out["bboxes"].index_select(0, rows), out["scores"].index_select(0, rows), info

    final_detections = staticmethod(final_detections)

    def fall_back(self, features_nchw, projections, tsdf, offset=None):
        """a scene that outgrew the size plan, through the eager path on the current stream (forward_scene: the true sizes are
        read back from the device); its sizes are kept in self.outgrown -- merged with those of earlier such scenes when they
        recorded the same sequence, in their place otherwise -- for rebuild(), and n_outgrown counts it.  Returns the eager result."""
        grown = P.Plan(self.margin)
        with P.using(grown):
            e = forward_scene(self.cfg, self.backbone, self.head, features_nchw, projections, tsdf, dense=self.dense,
                              offset=_offset_list(offset), keep_half=self.feature_dtype != torch.float32)
        prev = self.outgrown
        same = prev is not None and len(prev.sizes) == len(grown.sizes) and len(prev.flags) == len(grown.flags)
        self.outgrown = prev.merge(grown) if same else grown
        self.n_outgrown += 1
        return e

    def detect(self, features_nchw, projections, tsdf, rebuild_after=4, offset=None, by_reference=None):
        """run() + detections() with the fallback a server wants: a scene that outgrows the size plan (status != 0) is
        re-run through the eager path (sizes read back from the device) and its sizes are kept; after `rebuild_after`
        such scenes the plan is enlarged and the graph captured again (rebuild()), so a deployment whose scenes grew
        stops paying a replay plus an eager pass per scene.  Returns (bboxes, scores, info); info["static"] tells which
        path produced them."""
        out = self.run(features_nchw, projections, tsdf, offset=offset, by_reference=by_reference)
        try:
            with torch.cuda.stream(self.stream):          # the read-back waits on the stream the graph runs on
                b, s, info = self.detections(out)
            info["static"] = True
            return b, s, info
        except _lib.CnrmaError:
            with torch.cuda.stream(self.stream):
                e = self.fall_back(features_nchw, projections, tsdf, offset)
            info = {k: e[k] for k in ("M", "M_selected", "M_unique", "level_rows", "head_rows")}
            info["static"] = False
            if rebuild_after and self.n_outgrown >= rebuild_after:
                self.rebuild(features_nchw, projections, tsdf)
                info["rebuilt"] = True
            return e["bboxes"], e["scores"], info


class StaticBatch(_StaticGraph):
    """Several scenes per static pass: the geometric half (layout, dense unprojection, march, selection) per scene, then
    ONE collated multi-scene sparse tensor (batch id = scene, what ME.utils.batch_sparse_collate builds for B samples,
    ray_marching.py:328-330) through the backbone / neck / head, per-scene instance norm / pruning / decode with
    device-side row counts -- captured as ONE HIP graph.  The ~300 latency-bound launches of the network (35 of its 51
    convolutions run on < 12 k rows per scene) are thereby shared by the scenes of a pass.

    The size plan is derived from a calibrated SINGLE-scene plan (Plan.scaled): per-scene capacities for the geometric
    half, n_scenes x the single-scene capacities for the network."""

    def __init__(self, cfg, backbone, head, device, n_scenes, margin=1.2, dense=True, stream=None):
        super().__init__(device, margin, stream)
        self.cfg, self.backbone, self.head = cfg, backbone, head
        self.B, self.dense = int(n_scenes), dense
        # input holders: one StaticScene per scene of the pass, used for its static input buffers, its loader and its
        # geometric half only
        self.holders = [StaticScene(cfg, backbone, head, device, margin, dense, stream=self.stream) for _ in range(self.B)]

    def build(self, scenes, plan, capture=True):
        """scenes: B tuples (features_nchw, projections, tsdf[, offset]); plan: a calibrated single-scene Plan (merged over
        the scenes of the configuration, StaticScene.calibrate)."""
        _lib.require_gpu()
        assert len(scenes) == self.B
        self.plan = plan.scaled(self.B)
        self._enter(*(t for sc_ in scenes for t in (sc_[0], sc_[2])))       # feature maps and TSDFs, written just before build()
        with torch.cuda.stream(self.stream):
            for h, sc_ in zip(self.holders, scenes):
                h._alloc_inputs(sc_[0], sc_[2])
            self._load(scenes)
            self._capture(capture)

    def _load(self, scenes):
        for h, sc_ in zip(self.holders, scenes):
            h._load(sc_[0], sc_[1], sc_[2], None, sc_[3] if len(sc_) > 3 else None)

    def _trace(self):
        cfg, plan, B = self.cfg, self.plan, self.B
        plan.begin_static()
        out = {}
        with P.using(plan), torch.no_grad():
            vols, pts, Ms = [], [], []
            for b, h in enumerate(self.holders):                  # the geometric half, scene by scene
                dense, coords, feats, n_sel, info = h._geometry(seed=0x5EED + 7919 * b)
                vols.append(dense)
                pts.append((coords + h.offset_dev, feats, n_sel))
                Ms += [info["M"].view(1), n_sel.view(1)]
                if cfg.sample_seed is None:
                    h.seed_dev.add_(1)
            x = S.sparse_collate_static(pts, cfg.voxel_size_fcaf3d)
            levels = self.backbone(x)
            cen, box, cls, pt, css = map(list, self.head(levels, fused=True))
            bboxes, scores, valid, sizes = self.head.get_bboxes_static_multi(cen, box, cls, pt, css, B)
            status = plan.status(self.device)
            per_level = [l.cs.counts_dev()[0] for l in levels] + [c[0].counts_dev()[0] for c in css]
            counts = torch.cat(Ms + [x.cs.counts_dev()[0]] + per_level).to(torch.int32)
        plan.end_static()
        if self.dense:
            out.update(volume=[v[0] for v in vols], count=[v[1] for v in vols])
        out.update(bboxes=bboxes, scores=scores, valid=valid, sizes=sizes, status=status, counts=counts, n_levels=len(levels))
        return out

    def run(self, scenes):
        """enqueue one pass of B scenes on self.stream; returns the static output dict (valid until the next run)"""
        self._enter(*(t for sc_ in scenes for t in (sc_[0], sc_[2])))
        with torch.cuda.stream(self.stream):
            self._load(scenes)
            return self._replay()

    def detections(self, out):
        """static outputs -> [(bboxes, scores, info)] per scene; ONE device->host read for the whole pass"""
        B, L = self.B, len(out["sizes"])
        host = _read_back(out)
        valid, counts = host[:B * L], host[B * L:]
        nl = out["n_levels"]
        res = []
        for b in range(B):
            rows = _live_rows(out["sizes"], valid[b * L:(b + 1) * L], self.device)
            lv = counts[2 * B + B:]                               # after (M, M_sel) x B and the B unique counts
            info = dict(M=counts[2 * b], M_selected=counts[2 * b + 1], M_unique=counts[2 * B + b],
                        level_rows=[lv[l * B + b] for l in range(nl)], head_rows=[lv[(nl + l) * B + b] for l in range(nl)])
            res.append((out["bboxes"][b].index_select(0, rows), out["scores"][b].index_select(0, rows), info))
        return res


def gather_padded_detections(det, valid, det_all=None, valid_all=None):
    """ONE fixed-size exchange of a step's detections: det [S, K, W] = the padded raw boxes + scores of the
    S scenes a rank processed in the step, valid [S, L] = live rows per level.  Returns det_all [world, S, K, W] and
    valid_all [world, S, L].  No counts are read back: the padded blocks are small (<= 4000 x 25 floats per scene) and the
    row counts travel beside them.  Over RCCL (backend "nccl") this is two all_gather_into_tensor calls on device
    memory; other backends (gloo in the CPU / single-device tests) go through host lists."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return det.unsqueeze(0), valid.unsqueeze(0)
    W = dist.get_world_size()
    if det_all is None:
        det_all = torch.empty((W,) + tuple(det.shape), dtype=det.dtype, device=det.device)
        valid_all = torch.empty((W,) + tuple(valid.shape), dtype=valid.dtype, device=valid.device)
    if dist.get_backend() == "nccl":
        dist.all_gather_into_tensor(det_all, det)
        dist.all_gather_into_tensor(valid_all, valid)
    else:
        d, v = det.cpu(), valid.cpu()
        ds, vs = [torch.empty_like(d) for _ in range(W)], [torch.empty_like(v) for _ in range(W)]
        dist.all_gather(ds, d)
        dist.all_gather(vs, v)
        det_all.copy_(torch.stack(ds))
        valid_all.copy_(torch.stack(vs))
    return det_all, valid_all


def gather_detections(bboxes, scores):
    """variable-length all-gather of one scene's detections per rank over RCCL: first the row counts,
    then one padded [K_max, box+cls] block per rank.  Returns a list (per rank) of (bboxes, scores)."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return [(bboxes, scores)]
    W = dist.get_world_size()
    k = torch.tensor([bboxes.shape[0]], dtype=torch.int64, device=bboxes.device)
    ks = [torch.zeros_like(k) for _ in range(W)]
    dist.all_gather(ks, k)
    kmax = int(max(int(x.item()) for x in ks))
    nb, nc = bboxes.shape[1], scores.shape[1]
    block = torch.zeros((kmax, nb + nc), dtype=torch.float32, device=bboxes.device)
    block[:bboxes.shape[0], :nb] = bboxes
    block[:bboxes.shape[0], nb:] = scores
    blocks = [torch.empty_like(block) for _ in range(W)]
    dist.all_gather(blocks, block)
    return [(b[:int(n.item()), :nb], b[:int(n.item()), nb:]) for b, n in zip(blocks, ks)]
