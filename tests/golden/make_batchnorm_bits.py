"""Record tests/golden/batchnorm_bits.json: one SHA-256 per launch over the buffers it may write (and the status) of the twelve BatchNorm entries
(the nine vqa_bn_* entries that launch and the three that return counts) over the cases of tests/_bnbits.py.

Run on an MI355X with the library whose bits are to be pinned -- for a refactor, the PARENT commit's build (the C ABI is unchanged, so
it loads through the binding's LIB_PATH, as in tools/ab_lib.py):

    python tests/golden/make_batchnorm_bits.py [--lib tools/_build/libvqa_hip_parent.so] [--out tests/golden/batchnorm_bits.json]

Every case runs twice on fresh inputs; a digest that differs between the two passes refuses the recording.  Stored with the digests:
the `hipcc --version` line and the device name of the recording.  tests/test_gpu_batchnorm_bits.py recomputes the digests with the
product library and compares every one."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                          # tests/: _pkg, _optbits, _bnbits

import torch  # noqa: E402

import _bnbits as BB  # noqa: E402
from _pkg import sub  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build of libvqa_hip.so (default: the product library)")
    ap.add_argument("--out", default=os.path.join(HERE, "batchnorm_bits.json"))
    a = ap.parse_args()
    L = sub("_lib")
    if a.lib:
        L.LIB_PATH, L._lib = os.path.abspath(a.lib), None
    first = {k: fn() for k, fn in BB.cases().items()}
    second = {k: fn() for k, fn in BB.cases().items()}
    bad = [k for k in first if first[k] != second[k]]
    if bad:
        sys.exit("not reproducible, nothing written: " + ", ".join(bad))
    head = {"library": os.path.basename(L.LIB_PATH) if a.lib else "product", "hipcc": BB.toolchain(), "device": torch.cuda.get_device_name(0)}
    with open(a.out, "w") as f:                                    # one line per case
        f.write("{\n" + "".join(f" {json.dumps(k)}: {json.dumps(v)},\n" for k, v in sorted(head.items())))
        f.write(' "cases": {\n' + ",\n".join(f"  {json.dumps(k)}: {json.dumps(first[k], sort_keys=True)}" for k in sorted(first)) + "\n }\n}\n")
    print(f"{a.out}: {len(first)} cases, {sum(len(v) - 1 for v in first.values())} digests")


if __name__ == "__main__":
    main()
