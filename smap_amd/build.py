"""Build libsmap_hip.so (the gfx950 HIP library behind include/smap_hip.h) in-tree.

    python -m smap_amd.build [--force]

hipcc cross-compiles for gfx950 without a GPU.  The .so is git-ignored but travels
with the repo snapshot to the GPU box.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "libsmap_hip.so")
OBJ = os.path.join(CSRC, "obj")

# (source, extra flags).  assoc.hip, eval.hip, mupots.hip, labels.hip and loss.hip are bit-exact float work: contraction OFF.
SOURCES = [
    ("assoc.hip", ["-ffp-contract=off"]),
    ("eval.hip", ["-ffp-contract=off"]),
    ("mupots.hip", ["-ffp-contract=off"]),       # MuPoTS-3D protocol: float64 in a fixed order; its arithmetic is csrc/mupots_core.h (also built alone for the CPU)
    ("labels.hip", ["-ffp-contract=off"]),       # label maps: held to the reference's bits as well
    ("augment.hip", ["-ffp-contract=off"]),      # training samples: the warp's coordinate map in double, the resize of csrc/prep_device.h
    ("cubic_table.cpp", ["-ffp-contract=off"]),  # host-only C++: the bicubic remap's weight table (also built alone under sanitizers)
    ("loss.hip", ["-ffp-contract=off"]),         # training loss: fixed-order double sums; its finish is csrc/loss_core.h (also built alone for the CPU)
    ("heads.hip", ["-ffp-contract=off"]),        # head arms forward / backward in fp32: fixed-order MFMA chains, every other operation rounds once
    ("trunk.hip", ["-ffp-contract=off"]),        # Upsample_unit trunk forward / backward in fp32: the same GEMMs (csrc/gemm_f32_device.h) and the bilinear add
    ("conv.hip", []),
    ("conv3.hip", []),
    ("convp.hip", []),
    ("convf.hip", []),
    ("convb.hip", []),
    ("convc.hip", []),
    ("plan.hip", []),
    ("plan_check.cpp", []),       # host-only C++: which schedules and plan blobs the library runs (also built alone under sanitizers)
    ("jpeg.hip", []),
    ("jpeg_host.cpp", []),        # host-only C++ (marker parse + Huffman decode); no fast-math anywhere in this library
    ("jpeg_huff.hip", []),        # the Huffman decode on the device; its algorithm is csrc/jpeg_huff.h (also built alone for the CPU)
]
# -fvisibility=hidden: the .so exports exactly what include/smap_hip.h declares (its visibility push / pop), nothing of the internals
COMMON = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-I" + os.path.join(ROOT, "include"),
          "-I" + CSRC, "-Wall", "-Wno-unused-function"]


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError("hipcc not found")


def _newer(a, b):
    return (not os.path.exists(b)) or os.path.getmtime(a) > os.path.getmtime(b)


def build_lib(force=False, verbose=False):
    os.makedirs(OBJ, exist_ok=True)
    hipcc = _hipcc()
    headers = [os.path.join(ROOT, "include", "smap_hip.h")] + [
        os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".hpp", ".cuh"))]
    objs, relink = [], force
    for src, extra in SOURCES:
        sp = os.path.join(CSRC, src)
        if not os.path.exists(sp):
            continue
        op = os.path.join(OBJ, src.rsplit(".", 1)[0] + ".o")
        if force or _newer(sp, op) or any(_newer(h, op) for h in headers):
            cmd = [hipcc] + COMMON + extra + ["-c", sp, "-o", op]
            if verbose:
                print(" ".join(cmd), flush=True)
            subprocess.check_call(cmd)
            relink = True
        objs.append(op)
    if relink or not os.path.exists(OUT):
        # the dynamic symbol table = the functions include/smap_hip.h declares (-fvisibility=hidden + the header's visibility push) and
        # nothing else: a linker version script also keeps hipcc's per-unit __hip_cuid_* markers and weak template instantiations local
        vmap = os.path.join(OBJ, "exports.map")
        with open(vmap, "w") as f:
            f.write("{ global: smap_*; local: *; };\n")
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,--version-script=" + vmap, "-o", OUT] + objs
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return OUT


if __name__ == "__main__":
    print(build_lib(force="--force" in sys.argv, verbose=True))
