"""CN-RMA detector on the MI355X hot path.

Drop-in for the reference's projects/mvsdetection/models/ray_marching.py: same registered name (`RayMarching`),
same constructor keywords (:116-147), same method names and return contracts (forward / forward_test -> [{}],
train_step, val_step, parse_losses, data_converter, init_weights, aggregate_2d_features, clear_3d_features,
aggregate_2d_features_ray_marching, fcaf3d_detection, switch_pointcloud, ray_projection_neus/_depth) and the
module-level backproject() / get_ray_parameter().  All aggregation arithmetic runs in the HIP kernels of
cn-rma_amd/csrc through cnrma_amd.rma; the sparse detector runs on cnrma_amd.sparse.

Out of the hot-path scope: the 2D backbone (rows 7) and the Atlas 3D reconstruction network (row 6).
When their configs are None the detector takes their OUTPUTS as inputs: `features` [B][V,C,H',W'] and
`tsdf` (scene_tsdf_004, [B,1,X,Y,Z]) -- that is the synthetic-scene contract of bench.py.
"""
import os
import threading
import weakref
from collections import OrderedDict

import numpy as np
import torch
import torch.distributed as dist
from torch import nn

from cnrma_amd import rma
from cnrma_amd import sparse as S

from ..datasets.pipelines.fcaf3d_transforms import TransformFeaturesBBoxes, sample_points
from ..registry import DETECTORS, build_backbone, build_head
from .multiview_base import MultiViewBase


def backproject(voxel_dim, voxel_size, origin, projection, features):
    """Fill 2D features along camera rays into a voxel volume (reference :21-69).
    projection [B,3,4] (already stride-scaled), features [B,C,H,W] -> volume [B,C,nx,ny,nz], valid [B,1,nx,ny,nz] bool.
    One view per batch item, like the reference; the production path uses rma.backproject_accum for all views."""
    vols, valids = [], []
    org = origin.view(-1).tolist() if isinstance(origin, torch.Tensor) else list(origin)
    for b in range(features.shape[0]):
        nhwc = rma.to_nhwc(features[b:b + 1])
        vol, cnt = rma.backproject_accum(nhwc, projection[b:b + 1], voxel_dim, voxel_size, org, stride=1)
        vols.append(vol)
        valids.append((cnt > 0).unsqueeze(0))
    return torch.stack(vols), torch.stack(valids)


def get_ray_parameter(projection, features):
    """Ray origin / unit direction per feature-map pixel (reference :71-111): o, d [B,3,H*W]."""
    B, C, H, W = features.shape
    pinv = rma.projection_inverse(projection, 1).to(features.device)
    o, d = rma.ray_params(pinv, H, W)
    return o.unsqueeze(2).expand(B, 3, H * W).contiguous(), d


@DETECTORS.register_module()
class RayMarching(MultiViewBase):
    def __init__(self, pixel_mean, pixel_std, voxel_size, n_scales, voxel_dim_train, voxel_dim_test, origin,
                 backbone2d_stride, backbone2d, feature_2d, backbone_3d, tsdf_head, detection_backbone,
                 detection_head, feature_transform, save_path, loss_weight_recon=1.0, loss_weight_detection=1.0,
                 voxel_size_fcaf3d=0.01, use_batchnorm_train=True, use_batchnorm_test=True, max_points=None,
                 train_cfg=None, test_cfg=None, pretrained=None, use_feature_transform=True,
                 ray_marching_type="neus", depth_points=None, neus_threshold=None, middle_save_path=None,
                 middle_visualize_path=None, point_sampler="device", static_test=True, static_slots=3, static_calibration=2,
                 static_feature_handoff="reference", static_feature_dtype="float32", static_nms=None, mesh_extractor=None):
        super().__init__(pixel_mean, pixel_std, voxel_size, n_scales, voxel_dim_train, voxel_dim_test, origin, backbone2d_stride,
                         backbone2d, feature_2d, backbone_3d, tsdf_head, save_path, mesh_extractor=mesh_extractor)
        self.detection_backbone = build_backbone(detection_backbone)
        self.detection_head = build_head(detection_head)
        if not use_feature_transform:
            feature_transform = None
        self.feature_transform = TransformFeaturesBBoxes(**feature_transform) if feature_transform is not None else None
        self.voxel_size_fcaf3d = voxel_size_fcaf3d
        self.use_batchnorm_train = use_batchnorm_train
        self.use_batchnorm_test = use_batchnorm_test
        self.loss_weight_recon = loss_weight_recon
        self.loss_weight_detection = loss_weight_detection
        self.max_points = max_points
        self.ray_marching_type = ray_marching_type
        self.neus_threshold = neus_threshold
        self.depth_points = depth_points
        if ray_marching_type == "neus":
            assert neus_threshold is not None
        elif ray_marching_type == "depth":
            assert depth_points in [1, 2, 3, 4]
        self.middle_save_path = middle_save_path
        self.middle_visualize_path = middle_visualize_path
        # max_points subset of switch_pointcloud (:360-405): "device" (default) draws it on the GPU -- the same distribution as
        # the reference's np.random.choice from another random stream, no host RNG and no row count on the host, which is
        # what lets the shipped configs take the graph path below unmodified; "numpy" = the reference's global-RNG draw bit
        # for bit (parity switch: 45 ms of host time per ScanNet scene, ~1 s at the north-star shape, eager path only)
        if point_sampler not in ("device", "numpy"):
            raise ValueError(f"point_sampler must be 'device' or 'numpy', got {point_sampler!r}")
        self.point_sampler = point_sampler
        # inference fast path (forward_test): scenes of a repeating shape run as replayed HIP graphs, `static_slots` in
        # flight, the first `static_calibration` scenes eagerly (they size the graphs); see _forward_test_static
        self.static_test, self.static_slots, self.static_calibration = static_test, int(static_slots), int(static_calibration)
        self.static_margin = 1.2          # capacity = recorded size x margin (+ slack) of the graphs' size plan
        # how the fast path takes channels-last feature maps (pipeline.StaticScene.run): "reference" = the scene graph reads
        # the tensor the 2D stack (or the caller, for precomputed `features`) handed over, in place, until the scene has
        # left the GPU -- the producer must hand over a tensor it does not write again (a fresh allocation per scene, what
        # torch modules do; NOT a preallocated / double-buffered / graph-static output buffer); "copy" = copied into the
        # slot's own buffer first (+12.6 GB per slot and ~3.5 ms per scene at the north-star shape), nothing is assumed
        if static_feature_handoff not in ("reference", "copy"):
            raise ValueError(f"static_feature_handoff must be 'reference' or 'copy', got {static_feature_handoff!r}")
        self.static_feature_handoff = static_feature_handoff
        # element type of the graph path's feature maps: "float32" = everything is converted to fp32; "keep" = fp16 / bf16 maps
        # (a 2D stack run in half precision or under bf16 autocast; NeuS marching, C % 8 == 0) are handed over unconverted and
        # read in place -- same results bit for bit, no cast pass, half the slot buffer; slots are keyed by the maps' dtype
        if static_feature_dtype not in ("float32", "keep"):
            raise ValueError(f"static_feature_dtype must be 'float32' or 'keep', got {static_feature_dtype!r}")
        self.static_feature_dtype = static_feature_dtype
        # static_nms: None (default: the scene graphs end at the raw detections) or dict(score_thr=..., iou_thr=...): the per-class
        # NMS of post_process/nms_bbox.py runs at the end of every scene graph and the writer thread puts {scene}_atlas_bbox.npz
        # (boxes, scores, labels: the file nms_bbox.py writes) next to {scene}_bbox_raw.npz
        from cnrma_amd import pipeline as _pipeline
        self.static_nms = _pipeline.check_nms_setting(static_nms)
        self._static = {}
        self._writer = None
        import atexit
        ref = weakref.ref(self)

        def _flush_at_exit():
            m = ref()
            if m is not None:
                try:
                    m.flush()                 # results of the scenes still in flight when the test loop ended
                except Exception as e:       # the device may already be gone at interpreter exit: say so, do not raise
                    print(f"RayMarching: could not flush pending detections at exit: {e!r}")
        atexit.register(_flush_at_exit)
        self.initialize_volume()

    def initialize_volume(self):
        super().initialize_volume()
        self.points_detection = []

    # ---- the captured graphs hold raw pointers to prepared weight images: anything that may change the weights drops them ----
    def _reset_static(self):
        """write the results still in flight, then forget every captured graph (they are re-calibrated and re-captured by the
        next test scenes).  Called by train() / load_state_dict(): a train -> validate -> train loop, or a checkpoint load
        after the first test scene, must never replay weight images from build time."""
        if self.__dict__.get("_static"):
            try:
                self.flush()
            finally:
                self._static = {}
            self.__dict__["_lazy_points"] = None

    def train(self, mode=True):
        if mode != self.training or mode:
            self._reset_static()
        return super().train(mode)

    def _load_from_state_dict(self, *args, **kwargs):
        self._reset_static()
        return super()._load_from_state_dict(*args, **kwargs)

    def load_state_dict(self, *args, **kwargs):
        self._reset_static()
        return super().load_state_dict(*args, **kwargs)

    @property
    def points_detection(self):
        """the aggregated points of the last scene, [points [M,3+C]] (reference :289-307).  After a graph replay they sit
        in the slot's static buffers at capacity size; the list is cut to the live row count on first access (one
        device->host read) and is valid until that slot takes its next scene."""
        lazy = self.__dict__.get("_lazy_points")
        if lazy is not None:
            from cnrma_amd import pipeline
            out = lazy
            coords, _, n_dev = out["points"]
            torch.cuda.current_stream(coords.device).wait_event(out["done"])
            feats = pipeline.StaticScene.point_features(out)       # stored rows, or emitted now from the slot's point records
            n = int(n_dev.item())
            self.__dict__["_points"] = [torch.cat((coords[:n], feats[:n]), dim=1)]
            self.__dict__["_lazy_points"] = None
        return self.__dict__.get("_points", [])

    @points_detection.setter
    def points_detection(self, value):
        self.__dict__["_points"] = value
        self.__dict__["_lazy_points"] = None

    @property
    def valid(self):
        """[B,1,X,Y,Z] bool, `count > 0` of the dense unprojection (reference :247-257); after a graph replay it is derived
        from the slot's count volume on first access"""
        lazy = self.__dict__.get("_lazy_valid")
        if lazy is not None:
            count, done = lazy
            torch.cuda.current_stream(count.device).wait_event(done)
            self.__dict__["_valid"] = (count > 0).view(1, 1, *count.shape)
            self.__dict__["_lazy_valid"] = None
        return self.__dict__.get("_valid", 0)

    @valid.setter
    def valid(self, value):
        self.__dict__["_valid"] = value
        self.__dict__["_lazy_valid"] = None

    # ---- ray marching (reference :260-307, :687-956) ---------------------------------------------------------------
    def _rows(self, projection, features, tsdf, mode, thr=None, k=0, grids=300):
        B = features.shape[0]
        assert B == 1, "the reference is structurally batch-1 per GPU (ray_marching.py:707)"
        nhwc = rma.to_nhwc(features)
        pinv = rma.projection_inverse(projection.cpu(), 1).to(features.device)
        rows, per_view = rma.rma_view_rows(nhwc, pinv, tsdf[0, 0], self.voxel_dim, self.voxel_size,
                                           self.origin.view(-1).tolist(), grids, thr if thr is not None else 0.0, mode, k)
        return None if rows.shape[0] == 0 else [rows]

    def ray_projection_neus(self, projection, features, tsdf, grids=300, weight_threshold=None):
        """projection [B,3,4] stride-scaled, features [B,C,H,W], tsdf [B,1,X,Y,Z] -> [rows [M,4+C]] or None."""
        return self._rows(projection, features, tsdf, "neus", weight_threshold, 0, grids)

    def ray_projection_depth(self, projection, features, tsdf, grids=300, select_grids=None):
        return self._rows(projection, features, tsdf, "depth", None, select_grids, grids)

    def aggregate_2d_features_ray_marching(self, projections, features, tsdf):
        """projections [V,B,3,4] full-res, features [V,B,C,H,W], tsdf [B,1,X,Y,Z] -> self.points_detection =
        [points [M,3+C]] per scene (features scaled by w/mean(w))."""
        B = projections.shape[1]
        assert B == 1, "the reference is structurally batch-1 per GPU (ray_marching.py:707)"
        self.points_detection = []
        projections_cpu = projections.detach().cpu()                   # ONE device->host copy
        for b in range(B):
            pinv = rma.projection_inverse(projections_cpu[:, b], self.backbone2d_stride).to(features.device)
            # point_sampler="device": the max_points selection of switch_pointcloud (:360-405) is drawn on the GPU and fused
            # into the aggregation -- only the selected rows are emitted (the reference's numpy draw of 500 k out of
            # ~4 M indices alone costs 45 ms of host time per scene); "numpy" keeps the reference's RNG stream
            fused = self.point_sampler == "device" and self.max_points is not None and self.ray_marching_type == "neus"
            if torch.is_grad_enabled() and features.requires_grad and self.ray_marching_type in ("neus", "depth"):
                # training: the gradient of the aggregated features flows back into the 2D feature maps (:793-797, :947)
                coords, feats = rma.AggregatePoints.apply(features[:, b], pinv, tsdf[b, 0].detach(), self.voxel_dim,
                                                          self.voxel_size, self.origin.view(-1).tolist(), 300,
                                                          self.neus_threshold, (0.0, 0.0, 0.0),
                                                          self.max_points if fused else None,
                                                          "device" if fused else "numpy", None,
                                                          self.ray_marching_type, self.depth_points)
                self.points_detection.append(torch.cat((coords, feats), dim=1))
                continue
            nhwc = getattr(self, "_nhwc", {}).get((features.data_ptr(), b))      # the dense half's layout pass, if it ran on
            if nhwc is None:                                                     # these very feature maps
                nhwc = rma.to_nhwc(features[:, b])
            if fused:
                coords, feats, _ = rma.aggregate_points(nhwc, pinv, tsdf[b, 0], self.voxel_dim, self.voxel_size,
                                                        self.origin.view(-1).tolist(), 300, self.neus_threshold, "neus", 0,
                                                        (0.0, 0.0, 0.0), self.max_points, "device")
                self.points_detection.append(torch.cat((coords, feats), dim=1))
                continue
            pts, _ = rma.aggregate_rows(nhwc, pinv, tsdf[b, 0], self.voxel_dim, self.voxel_size,
                                        self.origin.view(-1).tolist(), 300, self.neus_threshold,
                                        self.ray_marching_type, self.depth_points)
            self.points_detection.append(pts)

    # ---- detection (reference :322-407) ------------------------------------------------------------------------------
    def switch_pointcloud(self, points, gt_bboxes, offsets, test):
        coords, feats, new_gt = [], [], []
        for b in range(len(points)):
            mask = None
            if self.max_points is not None and points[b].shape[0] > self.max_points:
                mask = sample_points(points[b], max_points=self.max_points)        # numpy global RNG, like the reference
            off = offsets[b].view(-1).tolist()
            if torch.is_grad_enabled() and points[b].requires_grad:      # training: keep the autograd graph of the features
                keep = points[b] if mask is None else points[b].index_select(
                    0, torch.nonzero(torch.as_tensor(mask, device=points[b].device)).view(-1))
                c, f = keep[:, :3].detach() + points[b].new_tensor(off), keep[:, 3:]
            else:
                c, f = rma.select_rows(points[b], off, mask)
            gt = gt_bboxes[b] if gt_bboxes is not None else None
            if self.feature_transform is not None and not test:
                c, gt = self.feature_transform(c, gt)
            coords.append(c)
            feats.append(f)
            new_gt.append(gt)
        return coords, feats, new_gt

    def fcaf3d_detection(self, inputs, points, test=False):
        coords, feats, gts = self.switch_pointcloud(points, inputs.get("gt_bboxes_3d"), inputs["offset"], test)
        x = S.sparse_collate(list(zip(coords, feats)), self.voxel_size_fcaf3d)
        levels = self.detection_backbone(x)
        centernesses, bbox_preds, cls_scores, pts = map(list, self.detection_head(levels))
        losses = {}
        if self.detection_head.loss_cls is not None and inputs.get("gt_bboxes_3d") is not None:
            losses = self.detection_head.loss(centernesses, bbox_preds, cls_scores, pts, gts, inputs["gt_labels_3d"])
        if test:
            self.last_detections = self.detection_head.get_bboxes(centernesses, bbox_preds, cls_scores, pts,
                                                                  inputs.get("scene"), self.save_path)
        return losses

    # ---- top level (reference :409-521) -----------------------------------------------------------------------------
    def _run(self, inputs, test):
        self.voxel_dim = self.voxel_dim_test if test else self.voxel_dim_train
        self.initialize_volume()
        projections = inputs["projection"].transpose(0, 1)
        features = self._features(inputs, self.use_batchnorm_test if test else self.use_batchnorm_train)
        self._view_source = (projections, features)       # the loop below hands out their rows: clear_3d_features re-uses them
        for projection, feature in zip(projections, features):
            self.aggregate_2d_features(projection, feature)
        self.clear_3d_features()
        recon_loss, recon_result = {}, None
        if self.backbone3d is not None:
            recon_result, recon_loss = self.tsdf_head(self.backbone3d(self.volume), inputs.get("tsdf_list"))
            tsdf = recon_result["scene_tsdf_004"]
        elif "tsdf" in inputs:
            tsdf = inputs["tsdf"]
        else:                                            # no 3D network and no TSDF input: march on the ground truth
            tsdf = inputs["tsdf_list"]["tsdf_gt_004"]
        self._last_tsdf = tsdf
        self.aggregate_2d_features_ray_marching(projections, features, tsdf)
        self._nhwc = {}
        detection_loss = self.fcaf3d_detection(inputs, self.points_detection, test=test)
        losses = {k: v * self.loss_weight_recon for k, v in recon_loss.items()}
        losses.update({k: v * self.loss_weight_detection for k, v in detection_loss.items()})
        if test and recon_result is not None and self.save_path is not None:
            results = self.save_reconstruction(recon_result, inputs)                         # {scene}.npz (+ .ply)
            if self.middle_save_path is not None and results:
                self.save_middle_result(results[0]["scene"], self.points_detection[0], results[0]["scene_tsdf"].origin,
                                        self.middle_save_path, self.middle_visualize_path)
        return losses

    def forward_train(self, inputs):
        return self._run(inputs, test=False)

    def forward_test(self, inputs):
        """reference :456-521.  On the graph path (see _forward_test_static) precomputed `features` that are channels-last in
        memory are read IN PLACE by the scene's graph until the scene has left the GPU (flush() / the scene's result file):
        do not overwrite that tensor before then, or construct the detector with static_feature_handoff="copy"."""
        if self._static_eligible(inputs):
            with torch.no_grad():
                self._forward_test_static(inputs)
        else:
            self.flush()
            self._run(inputs, test=True)
        return [{}]

    # ---- inference fast path: the scene as one replayed HIP graph (cnrma_amd.pipeline.StaticScene) ----------------------
    def _static_eligible(self, inputs):
        """The graph path takes a scene when nothing in it needs the host: NeuS or depth marching, the max_points subset drawn on
        the device (point_sampler="device"; the reference's numpy draw needs the row count on the host), one sample per
        GPU (the reference's own structural limit, ray_marching.py:707), eval mode.  Everything else -- and every scene
        that outgrows the size plan -- goes through the eager path (_run)."""
        if not self.static_test or self.training or self.ray_marching_type not in ("neus", "depth"):
            return False
        if self.max_points is not None and self.point_sampler != "device":
            return False
        if self.ray_marching_type == "neus" and (self.neus_threshold is None or self.neus_threshold <= 1.0 / 62):
            return False
        proj = inputs.get("projection")
        if proj is None or proj.shape[0] != 1:
            return False
        if self.fpn is None:
            f = inputs.get("features")
            f0 = f[0] if isinstance(f, (list, tuple)) else f
            if f0 is None or not f0.is_cuda:
                return False
        if self.middle_save_path is not None:
            return False
        return True

    def _forward_test_static(self, inputs):
        """forward_test (reference :456-521) without a host round trip per stage: feature maps [V,C,H',W'] are used where
        they lie (no stack copy, one layout pass inside the slot), the projections come to the host once, the TSDF is
        either an input or the Atlas network's output on the dense volume, and aggregation + FCAF3D + decode of the scene
        are ONE graph replay on one of `static_slots` streams.  Up to static_slots scenes are in flight, so the device never
        waits for the host between scenes; a writer thread puts {scene}_bbox_raw.npz on disk as soon as the scene's graph
        has finished (flush() waits for the ones still in flight)."""
        from cnrma_amd import pipeline
        self.voxel_dim = self.voxel_dim_test
        if self.fpn is None:
            f = inputs["features"]
            feats = f[0] if isinstance(f, (list, tuple)) else f[:, 0]                        # [V,C,H',W'] of sample 0
        else:
            images = inputs["imgs"][0]                                                        # [V,3,H,W]
            if self.use_batchnorm_test:
                feats = self.backbone2d(self.normalizer(images))
            else:
                feats = torch.cat([self.backbone2d(self.normalizer(im[None])) for im in images], dim=0)
        proj = inputs["projection"][0].detach().to("cpu", torch.float32)                      # ONE device->host copy per scene
        offset = inputs["offset"][0] if "offset" in inputs else None
        scene = inputs["scene"][0] if inputs.get("scene") is not None else None
        org = self.origin.view(-1).tolist()
        dense_in_graph = self.backbone3d is None
        fdt = torch.float32
        if (self.static_feature_dtype == "keep" and feats.dtype in rma.ELEM_CODES and feats.shape[1] % 8 == 0
                and self.ray_marching_type == "neus"):
            fdt = feats.dtype
        key = (tuple(feats.shape), tuple(self.voxel_dim), dense_in_graph, str(feats.device), str(fdt))
        ctx = self._static.get(key)
        if ctx is not None and ctx["built"] and ctx["tag"] != pipeline.weights_tag(ctx["weights"]):
            # an optimiser step / in-place weight update since the capture: the graphs would replay stale weight images
            self.flush()
            del self._static[key]
            ctx = None
        if ctx is None:
            cfg = pipeline.SceneConfig(self.voxel_dim, self.voxel_size, org, self.backbone2d_stride, 300,
                                       self.neus_threshold if self.ray_marching_type == "neus" else 0.05,
                                       self.max_points, self.voxel_size_fcaf3d, self.ray_marching_type, self.depth_points, "device")
            first = pipeline.StaticScene(cfg, self.detection_backbone, self.detection_head, feats.device, margin=self.static_margin,
                                         dense=dense_in_graph, by_reference=self.static_feature_handoff == "reference",
                                         feature_dtype=fdt, nms=self.static_nms)
            ctx = dict(cfg=cfg, slots=[first], pending=[None] * max(1, self.static_slots), seen=0, k=0, built=False,
                       weights=pipeline.weight_tensors(self.detection_backbone, self.detection_head), tag=None)
            self._static[key] = ctx
        if not ctx["built"]:
            # calibration scenes: the eager path produces their results (files, module state) exactly as before; a second,
            # recording pass over the same inputs sizes the graphs (its detections are dropped)
            self._run(inputs, test=True)
            self._save_final(*self.last_detections[0], scene)
            tsdf = self._last_tsdf.reshape(tuple(self.voxel_dim))
            first = ctx["slots"][0]
            first.calibrate(feats, proj, tsdf, offset=offset)
            ctx["seen"] += 1
            if ctx["seen"] >= max(1, self.static_calibration):
                self._build_slots(ctx, feats, proj, tsdf, dense_in_graph)
            return
        i = ctx["k"] % len(ctx["slots"])
        ctx["k"] += 1
        self._drain(ctx, i)                                     # the slot's previous scene leaves its buffers first
        st = ctx["slots"][i]
        recon_result, loaded = None, False
        if not dense_in_graph:
            # the Atlas 3D network sits between the two halves (:313-318): dense volume (one kernel) -> torch modules -> TSDF.
            # The layout pass writes straight into the static buffer of the slot this scene runs on.
            keep = st.feature_dtype != torch.float32         # 16-bit slot: the maps stay 16-bit here as well
            if rma.is_channels_last(feats, (st.feature_dtype,)):     # the 2D network's own layout: read in place, nothing to convert
                nhwc = rma.to_nhwc(feats, keep_dtype=keep)
            else:
                nhwc = rma.to_nhwc(feats, out=st._nhwc_buffer(), keep_dtype=keep)
                loaded = True
            vol, cnt = rma.backproject_accum(nhwc, proj, self.voxel_dim, self.voxel_size, org, self.backbone2d_stride)
            self.volume, self.valid = vol.unsqueeze(0), (cnt > 0).view(1, 1, *cnt.shape)
            recon_result, _ = self.tsdf_head(self.backbone3d(self.volume), inputs.get("tsdf_list"))
            tsdf = recon_result["scene_tsdf_004"]
        elif "tsdf" in inputs:
            tsdf = inputs["tsdf"]
        else:
            tsdf = inputs["tsdf_list"]["tsdf_gt_004"]
        tsdf = tsdf.reshape(tuple(self.voxel_dim))
        out = st.run(None if loaded else feats, proj, tsdf, offset=offset)
        if dense_in_graph:
            # module state as the eager path leaves it (:247-257): volume [B,C,X,Y,Z], valid [B,1,X,Y,Z] = count > 0 (lazily:
            # one elementwise kernel on the slot's stream when somebody reads it)
            self.volume = out["volume"].unsqueeze(0)
            self.__dict__["_lazy_valid"] = (out["count"], out["done"])
        self.__dict__["_lazy_points"] = out
        item = dict(out=out, scene=scene, inputs=(feats, proj, tsdf, offset), finished=threading.Event(), status=None,
                    result=None)
        ctx["pending"][i] = item
        self._writer_queue().put(item)                          # {scene}_bbox_raw.npz is written as soon as the scene has left the GPU
        if recon_result is not None and self.save_path is not None:
            self.save_reconstruction(recon_result, inputs)

    def _build_slots(self, ctx, feats, proj, tsdf, dense_in_graph, first_is_built=False):
        """capture the `static_slots` scene graphs at the plan's capacities (the first slot calibrated / re-planned them)"""
        from cnrma_amd import pipeline
        first = ctx["slots"][0]
        if not first_is_built:
            first.build(feats, proj, tsdf)
        ctx["slots"] = [first]
        for _ in range(1, max(1, self.static_slots)):
            st = pipeline.StaticScene(ctx["cfg"], self.detection_backbone, self.detection_head, feats.device, margin=first.margin,
                                      dense=dense_in_graph, by_reference=first.by_reference, feature_dtype=first.feature_dtype,
                                      nms=first.nms)
            st.build(feats, proj, tsdf, plan=first.plan)
            ctx["slots"].append(st)
        ctx["built"] = True
        ctx["tag"] = pipeline.weights_tag(ctx["weights"])

    # ---- results leave the device on a writer thread: a scene's file exists as soon as its graph has finished ---------------
    def _writer_queue(self):
        """Lazily started daemon thread: waits for a scene's `done` event (blocking only itself), reads the detections with ONE
        device->host copy on its own stream and writes {scene}_bbox_raw.npz (fcaf3d_head.py:266-271 writes it inside
        forward_test; here it lands a few hundred microseconds after the scene's last kernel instead of at slot reuse, so a
        crash loses at most the scenes still on the GPU).  Plan violations are left to the main thread (_drain)."""
        if self._writer is None or not self._writer[1].is_alive():
            import queue
            q = queue.Queue()
            t = threading.Thread(target=self._writer_loop, args=(q, weakref.ref(self)), name="cnrma-result-writer", daemon=True)
            t.start()
            self._writer = (q, t)
        return self._writer[0]

    @staticmethod
    def _writer_loop(q, ref):
        import queue
        from cnrma_amd import _lib, pipeline
        stream = None
        while True:
            try:
                item = q.get(timeout=5.0)
            except queue.Empty:
                if ref() is None:                                # the detector is gone: so is this thread
                    return
                continue
            if item is None:
                return
            try:
                out = item["out"]
                dev = out["bboxes"].device
                torch.cuda.set_device(dev)
                if stream is None:
                    stream = torch.cuda.Stream(device=dev)
                out["done"].synchronize()                        # blocks this thread only
                with torch.cuda.stream(stream), torch.no_grad():
                    b, s, _ = pipeline.StaticScene.detections(out)
                    b, s = b.cpu(), s.cpu()
                    final = None
                    if "nms_n" in out:                           # static_nms: the graph ended with the per-class NMS
                        final = [t.cpu().numpy() for t in pipeline.StaticScene.final_detections(out)]
                model = ref()
                if model is not None:
                    model._write_raw(b.numpy(), s.numpy(), item["scene"])
                    if final is not None:
                        model._write_final(*final, item["scene"])
                item["result"], item["status"] = (b, s), "ok"
            except _lib.CnrmaError:
                item["status"] = "violation"                     # outgrew the size plan: the main thread re-runs it eagerly
            except Exception as e:                              # noqa: BLE001 -- reported by _drain on the main thread
                item["status"], item["error"] = "error", e
            finally:
                item["finished"].set()
                # nothing of a finished scene -- its static buffers, the detector itself -- may outlive it in this frame: the
                # thread blocks in q.get() between scenes, and a name still bound here kept the last detector and its graphs
                # (tens of GB at the north-star shape) alive after `del model` (round 6: bench.py's resident memory)
                item = out = model = b = s = final = None

    def _drain(self, ctx, i, rebuild=True):
        """the slot's previous scene has left its static buffers (its file is written) -- or, if it outgrew the size plan,
        is re-run eagerly here (StaticScene.fall_back of the context's first slot, which keeps the sizes and the count);
        after 4 such scenes the plan is enlarged by their sizes and the graphs are captured again"""
        item = ctx["pending"][i]
        if item is None:
            return
        ctx["pending"][i] = None
        item["finished"].wait()
        if item["status"] == "ok":
            b, s = item["result"]
            self.last_detections = [(b, s)]
            return
        if item["status"] == "error":
            raise item["error"]
        self.static_fallbacks = getattr(self, "static_fallbacks", 0) + 1
        feats, proj, tsdf, offset = item["inputs"]
        first = ctx["slots"][0]
        e = first.fall_back(feats, proj, tsdf, offset)          # the eager pass reads the true sizes back and records them
        self._save_raw(e["bboxes"], e["scores"], item["scene"])
        if rebuild and first.n_outgrown >= 4:                   # a deployment whose scenes grew: stop paying replay + eager per scene
            for j in range(len(ctx["pending"])):
                if j != i:
                    self._drain_no_rebuild(ctx, j)
            first.rebuild(feats, proj, tsdf)
            self._build_slots(ctx, feats, proj, tsdf, first.dense, first_is_built=True)
            self.static_rebuilds = getattr(self, "static_rebuilds", 0) + 1

    def _drain_no_rebuild(self, ctx, j):
        self._drain(ctx, j, rebuild=False)                      # scenes drained on the way to a rebuild never trigger another one

    def flush(self):
        """wait until the detections of every scene still in flight are written (called when the eager path takes over, on
        train() / load_state_dict(), at interpreter exit, and by callers that read the result files right after the loop)"""
        for ctx in self._static.values():
            for i in range(len(ctx["pending"])):
                self._drain(ctx, i)

    def _write_raw(self, bboxes, scores, scene):
        if self.save_path is not None and scene is not None:
            d = os.path.join(self.save_path, scene)
            os.makedirs(d, exist_ok=True)
            final = os.path.join(d, scene + "_bbox_raw.npz")
            tmp = final + f".tmp{os.getpid()}.npz"
            np.savez(tmp, bboxes=bboxes, scores=scores)          # fcaf3d_head.py:266-271; renamed into place: a reader (or a crash)
            os.replace(tmp, final)                               # never sees a half-written file

    def _write_final(self, boxes, scores, labels, scene):
        """{scene}_atlas_bbox.npz as post_process/nms_bbox.py writes it (static_nms)"""
        if self.save_path is not None and scene is not None:
            d = os.path.join(self.save_path, scene)
            os.makedirs(d, exist_ok=True)
            final = os.path.join(d, scene + "_atlas_bbox.npz")
            tmp = final + f".tmp{os.getpid()}.npz"
            np.savez(tmp, boxes=boxes, scores=scores, labels=labels)
            os.replace(tmp, final)

    def _save_raw(self, bboxes, scores, scene):
        self.last_detections = [(bboxes, scores)]
        self._write_raw(bboxes.detach().cpu().numpy(), scores.detach().cpu().numpy(), scene)
        self._save_final(bboxes, scores, scene)

    def _save_final(self, bboxes, scores, scene):
        """static_nms for a scene that did not run as a graph (calibration scenes, scenes that outgrew the plan): the same file"""
        if self.static_nms is not None and self.save_path is not None and scene is not None:
            from cnrma_amd import postprocess
            final = postprocess.nms_device(bboxes.detach(), scores.detach(), **self.static_nms)
            self._write_final(*[t.cpu().numpy() for t in final], scene)

    def save_middle_result(self, scene_id, coords, offset, save_path, visualize_path=None):
        """dump the aggregated points of a scene ([M, 3 + C], coordinates moved by `offset`, at most max_points rows drawn
        like sample_points) as {scene}_vert.npy: the "middle" data the FCAF3D pre-training configs read
        (reference :959-991)"""
        pts = coords.detach().cpu().clone()
        pts[:, :3] += torch.as_tensor(offset).detach().cpu().view(1, 3)
        if self.max_points is not None and pts.shape[0] > self.max_points:
            keep = np.zeros(pts.shape[0], dtype=bool)
            keep[np.random.choice(pts.shape[0], self.max_points, replace=False)] = True
            pts = pts[torch.from_numpy(keep)]
        os.makedirs(save_path, exist_ok=True)
        np.save(os.path.join(save_path, scene_id + "_vert.npy"), pts.numpy())
        if visualize_path is not None:                       # ASCII .ply of the positions (the reference uses open3d)
            d = os.path.join(visualize_path, scene_id)
            os.makedirs(d, exist_ok=True)
            with open(os.path.join(d, scene_id + "_points.ply"), "w") as f:
                f.write(f"ply\nformat ascii 1.0\nelement vertex {pts.shape[0]}\nproperty float x\nproperty float y\n"
                        "property float z\nend_header\n")
                np.savetxt(f, pts[:, :3].numpy(), fmt="%.6f")
