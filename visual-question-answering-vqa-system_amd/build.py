"""Build libvqa_hip.so (gfx950) in-tree with hipcc.  `python build.py` or build_lib() from __graft_entry__.build()."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
# (optim_ops.hip, loss_ops.hip and attention.hip were split off token_ops.hip; they are linked last, in the order they were split off, so that
#  every other object keeps its place: profiles/optimizer_tail_ab.txt C, profiles/loss_ops_ab.txt C, profiles/attention_ab.txt C;
#  explain_ops.hip is new and goes last for the same reason: profiles/explain_ab_parent.txt; batchnorm.hip was split off cnn_ops.hip and goes
#  last in the same way: profiles/batchnorm_ab.txt C; bank_ops.hip is new and goes last: profiles/image_bank_ab_parent.txt; stats_ops.hip
#  is new and goes last: profiles/tensor_stats_ab_parent.txt)
SOURCES = ["gemm_conv.hip", "cnn_ops.hip", "token_ops.hip", "stem_conv.hip", "conv_c64.hip", "input_ops.hip", "gemm8p.hip", "mxfp8.hip", "stem_dgrad.hip", "feature_ops.hip", "optim_ops.hip", "loss_ops.hip", "attention.hip", "explain_ops.hip", "batchnorm.hip", "bank_ops.hip", "stats_ops.hip"]
HEADER = os.path.join(os.path.dirname(HERE), "include", "vqa_hip.h")
LIB = os.path.join(HERE, "libvqa_hip.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result"]


def _deps():
    """Every file the library is compiled from: the sources, the headers next to them, and the public header common.h includes."""
    import glob
    return [os.path.join(CSRC, f) for f in SOURCES] + glob.glob(os.path.join(CSRC, "*.h")) + [HEADER]


def _stale():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    return any(os.path.getmtime(d) > t for d in _deps())


def build_lib(force=False, verbose=True):
    if not force and not _stale():
        return LIB
    objs = []
    procs = []
    for src in SOURCES:
        obj = os.path.join(CSRC, src.replace(".hip", ".o"))
        objs.append(obj)
        cmd = [HIPCC] + FLAGS + ["-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        procs.append((cmd, subprocess.Popen(cmd)))
    for cmd, p in procs:
        if p.wait() != 0:
            raise RuntimeError("hipcc failed: " + " ".join(cmd))
    cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    build_lib(force="--force" in sys.argv)
    print(LIB)
