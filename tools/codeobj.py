"""The gfx950 code object inside a built object or library (development tools): the one
unbundling that tools/isa.py, tools/kernel_resources.py and tools/codeobj_diff.py share."""
import contextlib
import os
import subprocess
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


def llvm(tool, *args):
    """stdout of an LLVM binutil run on `args` (raises when it fails)."""
    return subprocess.run([f"{LLVM}/{tool}", *args], capture_output=True, text=True, check=True).stdout


@contextlib.contextmanager
def code_object(path):
    """Path of the gfx950 code object unbundled from `path`'s .hip_fatbin (a temporary file).
    A linked library bundles one code object per translation unit and the unbundler reads the
    first only: pass the build's objects (build/obj/<lib>/*.o) to see every kernel."""
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "k.co")
        llvm("llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", path)
        llvm("clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}",
             "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}")
        yield co
