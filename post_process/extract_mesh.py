"""Meshes of the TSDF volumes the detectors wrote ({scene}/{scene}.npz -> {scene}/{scene}.ply), by the library's marching cubes on
the GPU (cnrma_amd.mesh).  For volumes that are already on disk: a run with mesh_extractor="device" writes the same file itself.
The .ply is what the reference's post_process/evaluate_mesh.py and visualize_results.py start from."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from projects.mvsdetection.datasets.tsdf import TSDF  # noqa: E402


def extract_meshes(args):
    for scene_id in sorted(os.listdir(args.result_path)):
        npz = os.path.join(args.result_path, scene_id, scene_id + ".npz")
        if not os.path.isfile(npz):
            continue
        tsdf = TSDF.load(npz).to("cuda")
        tsdf.get_mesh_device().export(os.path.join(args.result_path, scene_id, scene_id + args.postfix))
        print("Saved", scene_id)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--result_path", type=str, required=True)
    ap.add_argument("--postfix", type=str, default=".ply")
    extract_meshes(ap.parse_args())
