"""Scores the reconstructed meshes ({result_path}/{scene}/{scene}.ply) against the ground-truth meshes: accuracy, completeness,
precision, recall and F-score at 5 cm after a 2 cm voxel down-sample, on the GPU (cnrma_amd.cloud).  The reference's
post_process/evaluate_mesh.py with its arguments, file layout and metrics.json, without Open3D."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KEY_NAMES = ["dist1", "dist2", "prec", "recal", "fscore"]


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", type=str, default="arkit", choices=["scannet", "arkit"])
    ap.add_argument("--data_path", type=str, required=True)
    ap.add_argument("--result_path", type=str, required=True)
    ap.add_argument("--axis_align", type=int, default=1)
    return ap.parse_args(argv)


def read_axis_align_matrix(path):
    """the 4x4 `axisAlignment = ...` of a ScanNet scene's .txt (identity when the file or the line is missing)"""
    m = np.eye(4)
    if os.path.exists(path):
        for line in open(path):
            if "axisAlignment" in line:
                m = np.array([float(x) for x in line.split("=", 1)[1].split()], dtype=np.float64).reshape(4, 4)
                break
    return m


def scene_files(args, scene_id):
    """-> (predicted .ply, ground-truth .ply, axis-alignment matrix or None)"""
    pred = os.path.join(args.result_path, scene_id, scene_id + ".ply")
    if args.dataset == "scannet":
        scan = os.path.join(args.data_path, "scans", scene_id)
        m = read_axis_align_matrix(os.path.join(scan, scene_id + ".txt")) if args.axis_align else None
        return pred, os.path.join(scan, scene_id + "_vh_clean_2.ply"), m
    return pred, os.path.join(args.data_path, "3dod", "Validation", scene_id, scene_id + "_3dod_mesh.ply"), None


def scene_names(args):
    if args.dataset == "scannet":
        names = [line.rstrip() for line in open(os.path.join(args.data_path, "meta_data", "scannetv2_val.txt"))]
    else:
        names = os.listdir(os.path.join(args.data_path, "3dod", "Validation"))
    return sorted(n for n in names if n)


def load_scene(args, scene_id):
    """-> (predicted points, ground-truth points) as float32 [N,3]; the axis alignment is applied to the ground truth in fp64
    and rounded to fp32"""
    from cnrma_amd import cloud
    pred_path, gt_path, m = scene_files(args, scene_id)
    pred, gt = cloud.read_ply_points(pred_path), cloud.read_ply_points(gt_path)
    if m is not None:
        gt = (gt.astype(np.float64) @ m[:3, :3].T + m[:3, 3]).astype(np.float32)
    return pred, gt


def display_results(metrics):
    for k in KEY_NAMES:
        vals = np.array([m[k] for m in metrics.values() if k in m], dtype=np.float64)
        print("%10s %0.3f" % (k, np.nanmean(vals) if len(vals) and not np.isnan(vals).all() else np.nan))


def evaluate_meshes(args):
    """scores every scene, writes {result_path}/metrics.json = {scene: {dist1, dist2, prec, recal, fscore}} and returns it"""
    from cnrma_amd import cloud
    metrics = {}
    for scene_id in scene_names(args):
        pred, gt = load_scene(args, scene_id)
        metrics[scene_id] = cloud.eval_mesh(pred, gt)
        print(scene_id, metrics[scene_id])
    with open(os.path.join(args.result_path, "metrics.json"), "w") as fh:
        json.dump(metrics, fh)
    display_results(metrics)
    return metrics


if __name__ == "__main__":
    evaluate_meshes(parse_args())
