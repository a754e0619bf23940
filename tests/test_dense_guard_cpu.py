"""CPU tests of what keeps the dense unprojection's build honest: the Python names of its A/B switches follow the order of the C
vector, and the build guard (scripts/kernel_resources.py --check) refuses a product kernel that spills, grows past its
register budget, loses occupancy, or is missing from the report."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIPE = "_ZN12_GLOBAL__N_129backproject_accum_pipe_kernelILi%dELi1ELi0ELi0EEEvNS_11DenseParamsEPKfS3_PfPiilNS_9SlabOrderEPjPKS3_"


def test_dense_tuning_names_follow_the_c_vector():
    from cnrma_amd import rma
    src = open(os.path.join(ROOT, "cn-rma_amd", "csrc", "dense.hip")).read()
    fields = re.search(r"int\* f\[\] = \{([^}]*)\};", src).group(1)
    names = tuple(n.strip().replace("&t.", "") for n in fields.split(","))
    assert names == rma._DENSE_KEYS
    assert names[-1] == "zrun"                                  # new switches are appended: older callers pass a shorter vector
    assert re.search(r"n > %d \|\|" % len(names), src)
    struct = src[src.index("struct DenseTune {"):src.index("};", src.index("struct DenseTune {"))]
    assert re.search(r"int zrun = 1;", struct)                   # the default is the z-run mapping


def _report(tmp_path, kernels):
    lines = []
    for lpv, vgpr, scratch, occ in kernels:
        head = "dense.hip:1:1: remark: "
        lines += [head + "Function Name: " + PIPE % lpv + " [-Rpass-analysis=kernel-resource-usage]",
                  head + "    VGPRs: %d [-Rpass-analysis=kernel-resource-usage]" % vgpr,
                  head + "    AGPRs: 0 [-Rpass-analysis=kernel-resource-usage]",
                  head + "    ScratchSize [bytes/lane]: %d [-Rpass-analysis=kernel-resource-usage]" % scratch,
                  head + "    Occupancy [waves/SIMD]: %d [-Rpass-analysis=kernel-resource-usage]" % occ,
                  head + "    LDS Size [bytes/block]: 0 [-Rpass-analysis=kernel-resource-usage]"]
    path = tmp_path / "dense.resources.txt"
    path.write_text("\n".join(lines) + "\n")
    return subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "kernel_resources.py"), "--check", str(path),
                           "backproject_accum_pipe_kernel", "<8, 1, 0, 0>:128:4"], capture_output=True, text=True)


def test_guard_accepts_the_budget_and_refuses_everything_else(tmp_path):
    ok = _report(tmp_path, [(8, 123, 0, 4), (4, 59, 0, 8)])
    assert ok.returncode == 0, ok.stdout + ok.stderr
    for bad in ([(8, 132, 0, 3), (4, 59, 0, 8)],        # over the register budget (and so below 4 waves per SIMD)
                [(8, 128, 0, 3), (4, 59, 0, 8)],        # occupancy lost
                [(8, 128, 16, 4), (4, 59, 0, 8)],       # the product instantiation spills
                [(8, 123, 0, 4), (4, 59, 8, 8)],        # another product instantiation spills
                [(4, 59, 0, 8)]):                       # the product instantiation is not in the report
        r = _report(tmp_path, bad)
        assert r.returncode != 0 and "FAILED" in r.stdout, (bad, r.stdout)
