"""In-tree hipcc build of the kubetorch_amd HIP extension (gfx950 only).

Produces kubetorch_amd/ops/_hip_ops.so next to this file so the built
artifact travels with the repo snapshot to GPU boxes (no JIT cache).

Invoked by __graft_entry__.build() and by `python -m kubetorch_amd.ops.build`.
"""
import os
import subprocess
import sys
import sysconfig

OPS_DIR = os.path.dirname(os.path.abspath(__file__))
HIP_DIR = os.path.join(OPS_DIR, "hip")
BUILD_DIR = os.path.join(OPS_DIR, "_build")
ARCH = os.environ.get("PYTORCH_ROCM_ARCH", "gfx950")

# module name -> sources (each builds an in-tree .so)
MODULES = {
    "_hip_ops": ["kernels.hip", "attention.hip", "attention_ck.hip", "attention_ck_bwd.hip", "paged_attention.hip", "paged_prefill.hip", "sampler.hip", "logprobs.hip", "linear_w8.hip", "bindings.cpp"],
    "_hip_spill": ["spill.cpp"],
}
SO_PATH = os.path.join(OPS_DIR, "_hip_ops.so")  # primary (back-compat)


def _torch_paths():
    import torch

    troot = os.path.dirname(torch.__file__)
    includes = [
        os.path.join(troot, "include"),
        os.path.join(troot, "include", "torch", "csrc", "api", "include"),
        sysconfig.get_paths()["include"],
    ]
    libdir = os.path.join(troot, "lib")
    return includes, libdir


def _common_flags(includes):
    flags = [
        f"--offload-arch={ARCH}",
        "-O3",
        "-std=c++17",
        "-fPIC",
        "-fno-gpu-rdc",
        "-DUSE_ROCM=1",
        "-DHIPBLAS_V2",
        "-DCUDA_HAS_FP16=1",
        "-D__HIP_NO_HALF_OPERATORS__=1",
        "-D__HIP_NO_HALF_CONVERSIONS__=1",
        "-DTORCH_API_INCLUDE_EXTENSION_H",
    ]
    import torch

    flags.append(
        "-D_GLIBCXX_USE_CXX11_ABI=" + ("1" if torch._C._GLIBCXX_USE_CXX11_ABI else "0")
    )
    for inc in includes:
        flags += ["-I", inc]
    return flags


def _needs_rebuild(so_path, sources):
    if not os.path.exists(so_path):
        return True
    so_mtime = os.path.getmtime(so_path)
    for src in sources + ["build.py"]:
        p = (os.path.join(HIP_DIR, src) if src != "build.py"
             else os.path.join(OPS_DIR, src))
        if os.path.getmtime(p) > so_mtime:
            return True
    return False


def _build_module(name, sources, verbose, force):
    so_path = os.path.join(OPS_DIR, name + ".so")
    if not force and not _needs_rebuild(so_path, sources):
        if verbose:
            print(f"[kubetorch_amd.ops.build] up to date: {so_path}")
        return so_path
    os.makedirs(BUILD_DIR, exist_ok=True)
    includes, libdir = _torch_paths()
    flags = _common_flags(includes) + [f"-DTORCH_EXTENSION_NAME={name}"]
    hipcc = os.environ.get("HIPCC", "hipcc")
    objs = []
    for src in sources:
        obj = os.path.join(BUILD_DIR, os.path.splitext(src)[0] + ".o")
        src_flags = flags
        if src in ("attention.hip", "attention_ck.hip", "attention_ck_bwd.hip"):
            # rocWMMA/ck_tile need the __half conversions torch's flags
            # disable; these TUs have no torch headers -> drop the guards.
            src_flags = [f for f in flags
                         if not f.startswith("-D__HIP_NO_HALF")]
        cmd = [hipcc, "-c", os.path.join(HIP_DIR, src), "-o", obj] + src_flags
        if verbose:
            print("[hipcc]", " ".join(cmd))
        subprocess.run(cmd, check=True)
        objs.append(obj)
    link = (
        [hipcc, "-shared", "-fPIC", "-o", so_path]
        + objs
        + [
            f"-L{libdir}",
            f"-Wl,-rpath,{libdir}",
            "-ltorch",
            "-ltorch_hip",
            "-ltorch_python",
            "-lc10",
            "-lc10_hip",
            "-lamdhip64",
        ]
    )
    if verbose:
        print("[hipcc link]", " ".join(link))
    subprocess.run(link, check=True)
    if verbose:
        print(f"[kubetorch_amd.ops.build] built {so_path}")
    return so_path


def build(verbose=True, force=False):
    """Compile every HIP extension module in-tree (idempotent)."""
    out = None
    for name, sources in MODULES.items():
        path = _build_module(name, sources, verbose, force)
        if name == "_hip_ops":
            out = path
    return out


if __name__ == "__main__":
    build(force="--force" in sys.argv)
