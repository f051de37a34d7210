"""Compile the reference's own CUDA NMS (eval/src/nms_cuda.cpp + nms_kernel.cu) for gfx950 into oracle/_ref/.

TEST INFRASTRUCTURE ONLY.  Runs only where the reference tree exists (the build container); the GPU box uses the
prebuilt oracle/_ref/*.so that travels with the snapshot.  Nothing of the reference lands in a tracked directory.

Recipe:
  1. stage   the two sources are written into oracle/_ref/nms_cuda_src/ through `sed`, with one edit: torch 2.10's
             at::globalContext().lazyInitCUDA() returns void, so `THCState *state = ...` becomes `= nullptr` (`state`
             only reaches the shim allocator).  The algorithm lines compile untouched.  The THC headers the kernel file
             includes (gone since torch 1.11) are our own stand-ins, oracle/thc_shim/, staged beside them.
  2. hipify  torch's hipify rewrites the staged tree in place (nms_kernel.hip beside the .cu, THH/THH.h in the shim).
  3. build   two modules from the same hipified text:
               nms_cuda_ref_exact  -ffp-contract=off: every operation rounds once, which is what the source states
               nms_cuda_ref_fused  hipcc's default contraction (devIoU's Sa + Sb - interS and friends become FMAs), the
                                   choice a fusing compiler such as nvcc -fmad=true may make
             both with -fno-slp-vectorize; the gfx950 assembly is kept and must pass orienmask_amd/csrc/isa_audit.py,
             like every product kernel, or the build fails.
"""
import os
import shutil
import subprocess
import sys
import sysconfig

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "_ref")
STAGE = os.path.join(OUT, "nms_cuda_src")
SHIM = os.path.join(HERE, "thc_shim")
AUDIT = os.path.join(HERE, "..", "orienmask_amd", "csrc", "isa_audit.py")
ARCH = "gfx950"
VARIANTS = {"exact": ["-ffp-contract=off"], "fused": []}
# the one edit (nms_kernel.cu:89)
SED_EDIT = r"s/THCState \*state = at::globalContext()\.lazyInitCUDA();/THCState *state = nullptr;/"


def module_path(variant):
    return os.path.join(OUT, "nms_cuda_ref_%s%s" % (variant, sysconfig.get_config_var("EXT_SUFFIX")))


def _inputs(ref_root):
    src = os.path.join(ref_root, "eval", "src")
    files = [os.path.join(src, "nms_cuda.cpp"), os.path.join(src, "nms_kernel.cu"), os.path.abspath(__file__), AUDIT]
    for d, _, names in os.walk(SHIM):
        files += [os.path.join(d, n) for n in names]
    return files


def _run(cmd, **kw):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, **kw)
    if r.returncode != 0:
        raise RuntimeError("oracle/_ref: failed (rc=%d): %s\n%s" % (r.returncode, " ".join(cmd), r.stdout[-4000:]))
    return r.stdout


def stage(ref_root):
    src = os.path.join(ref_root, "eval", "src")
    shutil.rmtree(STAGE, ignore_errors=True)
    os.makedirs(STAGE)
    with open(os.path.join(STAGE, "nms_cuda.cpp"), "w") as f:
        subprocess.check_call(["sed", "", os.path.join(src, "nms_cuda.cpp")], stdout=f)
    kernel = os.path.join(STAGE, "nms_kernel.cu")
    with open(kernel, "w") as f:
        subprocess.check_call(["sed", SED_EDIT, os.path.join(src, "nms_kernel.cu")], stdout=f)
    text = open(kernel).read()
    if "lazyInitCUDA" in text or "THCState *state = nullptr;" not in text:
        raise RuntimeError("oracle/_ref: the lazyInitCUDA edit did not apply to nms_kernel.cu")
    shutil.copytree(SHIM, os.path.join(STAGE, "shim"))


def hipify():
    from torch.utils.hipify import hipify_python
    shim = os.path.join(STAGE, "shim")
    res = hipify_python.hipify(project_directory=STAGE, output_directory=STAGE, header_include_dirs=[shim],
                               extra_files=[os.path.join(STAGE, "nms_cuda.cpp"), os.path.join(STAGE, "nms_kernel.cu")],
                               show_detailed=False, show_progress=False, is_pytorch_extension=True)
    out = {}
    for name in ("nms_cuda.cpp", "nms_kernel.cu"):
        p = os.path.join(STAGE, name)
        out[name] = res[p].hipified_path if p in res and res[p].hipified_path else p
    return out, shim


def build_variant(variant, sources, shim):
    import torch
    from torch.utils import cpp_extension
    bdir = os.path.join(STAGE, "build_" + variant)
    os.makedirs(bdir, exist_ok=True)
    inc = ["-I" + shim]
    for p in cpp_extension.include_paths(device_type="cuda"):
        inc += ["-isystem", p]
    inc += ["-isystem", sysconfig.get_paths()["include"]]
    abi = int(torch._C._GLIBCXX_USE_CXX11_ABI)
    defs = ["-DTORCH_EXTENSION_NAME=nms_cuda_ref_" + variant, "-DTORCH_API_INCLUDE_EXTENSION_H",
            "-D_GLIBCXX_USE_CXX11_ABI=%d" % abi, "-D__HIP_PLATFORM_AMD__=1", "-DUSE_ROCM=1", "-DHIPBLAS_V2",
            "-DCUDA_HAS_FP16=1", "-D__HIP_NO_HALF_OPERATORS__=1", "-D__HIP_NO_HALF_CONVERSIONS__=1"]
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    kobj = os.path.join(bdir, "nms_kernel.o")
    _run([hipcc, "--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-w", "-fno-gpu-rdc", "-fno-slp-vectorize",
          "-save-temps=obj"] + VARIANTS[variant] + defs + inc + ["-x", "hip", "-c", sources["nms_kernel.cu"], "-o", kobj],
         cwd=bdir)
    asm = [os.path.join(bdir, f) for f in os.listdir(bdir) if f.endswith("-hip-amdgcn-amd-amdhsa-%s.s" % ARCH)]
    if not asm:
        raise RuntimeError("oracle/_ref: no %s assembly kept for %s" % (ARCH, variant))
    _run([sys.executable, AUDIT] + asm)
    for f in os.listdir(bdir):      # keep the object and the audited device assembly, drop the other -save-temps products
        if f != "nms_kernel.o" and f not in [os.path.basename(a) for a in asm]:
            os.remove(os.path.join(bdir, f))
    cobj = os.path.join(bdir, "nms_cuda.o")
    _run(["g++", "-O2", "-std=c++17", "-fPIC", "-w"] + defs + inc + ["-c", sources["nms_cuda.cpp"], "-o", cobj], cwd=bdir)
    libdir = os.path.join(os.path.dirname(torch.__file__), "lib")
    rocm_lib = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")
    out = module_path(variant)
    _run([hipcc, "--offload-arch=" + ARCH, "-fno-gpu-rdc", "-shared", "-fPIC", kobj, cobj, "-o", out,
          "-L" + libdir, "-Wl,-rpath," + libdir, "-L" + rocm_lib, "-Wl,-rpath," + rocm_lib,
          "-lc10", "-lc10_hip", "-ltorch", "-ltorch_cpu", "-ltorch_hip", "-ltorch_python", "-lamdhip64"], cwd=bdir)
    return out, asm[0]


def fma_count(asm_path):
    return sum(1 for line in open(asm_path) if line.strip().startswith(("v_fma_f32", "v_fmac_f32", "v_fma_mix", "v_mad_f32")))


def main(ref_root):
    if not os.path.isfile(os.path.join(ref_root, "eval", "src", "nms_kernel.cu")):
        print("oracle/_ref: reference not present, CUDA NMS skipped")
        return 0
    newest_in = max(os.path.getmtime(p) for p in _inputs(ref_root))
    outs = [module_path(v) for v in VARIANTS]
    if all(os.path.exists(o) and os.path.getmtime(o) > newest_in for o in outs):
        print("oracle/_ref: nms_cuda_ref_{%s} up to date" % ",".join(VARIANTS))
        return 0
    os.makedirs(OUT, exist_ok=True)
    stage(ref_root)
    sources, shim = hipify()
    for v in VARIANTS:
        out, asm = build_variant(v, sources, shim)
        print("oracle/_ref: built %s (isa_audit passed; %d fma in the kernel)" % (os.path.basename(out), fma_count(asm)))
    return 0


if __name__ == "__main__":
    try:
        sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else "/root/reference"))
    except RuntimeError as e:
        print(e)
        sys.exit(1)
