"""Build recipe for the reference's own CPU pixel code: oracle/_ref/libcprocess_ref.so and libcprocess_ref_fma.so.

TEST INFRASTRUCTURE.  The reference's src/cprocess files are compiled where they lie; nothing of them is copied, patched or
committed.  What this recipe adds is its own: a stand-in <GL/glew.h> (oracle/ref_shim/) so that the GL halves of those files
compile, and a Python-3 conversion of the half-table generator, made with lib2to3 on a copy under oracle/_ref/ and run there.

  libcprocess_ref.so      gcc, the flags of oracle/Makefile's default target (-ffp-contract=off): checks liboracle.so
  libcprocess_ref_fma.so  the clang and the flags of that Makefile's `fma` target (-ffp-contract=on -mfma -mavx2, no
                          -march=native for the reason given there): checks liboracle_fma.so

GL entry points stay undefined in both; the CPU paths never reach them, and oracle.ref() loads the files with lazy binding.
tests/test_oracle_against_reference.py compares the restatement with these libraries bit for bit, and
tests/golden/make_reference_golden.py records their results for the GPU tests, which never see the reference.

Run `python3 oracle/ref_build.py` to build by hand; __graft_entry__.build() calls build() when available() holds.
"""
import os
import shutil
import subprocess
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = os.environ.get("CANVAS_REFERENCE_DIR", "/root/reference")
OUT_DIR = os.path.join(_HERE, "_ref")
SHIM = os.path.join(_HERE, "ref_shim")
CLANG = os.environ.get("CLANG", "/opt/rocm/lib/llvm/bin/clang")

FILES = ["half", "gammatab", "color", "filter", "video_mix", "video_scale", "video_filter", "video_reconstruct",
         "video_subsample", "workspace", "main", "audio_mix"]

COMMON = ["-O3", "-fno-math-errno", "-fPIC", "-w"]
FLAVOURS = {
    # name -> (file, compiler, flags); -std=gnu99 where oracle/Makefile says c99: the reference's files use POSIX and
    # glib declarations that the strict mode hides, the arithmetic is the same
    "gcc": ("libcprocess_ref.so", "gcc", ["-std=gnu99", "-fno-signed-zeros", "-ffp-contract=off"]),
    "fma": ("libcprocess_ref_fma.so", CLANG, ["-std=gnu99", "-ffp-contract=on", "-mfma", "-mavx2",
                                               "-Wno-error=implicit-function-declaration"]),
}


def src_dir():
    return os.path.join(REFERENCE, "src", "cprocess")


def glib_dirs():
    """(include, config include, lib) of a glib installation, or None."""
    for inc, cfg, lib in (("/usr/include/glib-2.0", "/usr/lib/x86_64-linux-gnu/glib-2.0/include", "/usr/lib/x86_64-linux-gnu"),
                          ("/opt/conda/include/glib-2.0", "/opt/conda/lib/glib-2.0/include", "/opt/conda/lib")):
        if os.path.exists(os.path.join(inc, "glib.h")) and os.path.exists(os.path.join(cfg, "glibconfig.h")):
            return inc, cfg, lib
    return None


def available():
    """The reference's sources and glib's headers are both here."""
    return os.path.isfile(os.path.join(src_dir(), "video_mix.c")) and glib_dirs() is not None


def path(flavour="gcc"):
    return os.path.join(OUT_DIR, FLAVOURS[flavour][0])


def _run(cmd, **kw):
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, **kw)
    if p.returncode != 0:
        raise RuntimeError("%s failed:\n%s" % (" ".join(cmd), p.stdout[-4000:]))
    return p.stdout


def _halftab():
    """SConstruct:109 runs the generator with Python 2; here a converted copy runs under this interpreter."""
    gen = os.path.join(OUT_DIR, "genhalf.py")
    shutil.copyfile(os.path.join(src_dir(), "genhalf.py"), gen)
    _run([sys.executable, "-m", "lib2to3", "-w", "-n", gen])
    out = os.path.join(OUT_DIR, "halftab.c")
    text = _run([sys.executable, gen])
    with open(out, "w") as f:
        f.write(text)
    return out


def build(force=False):
    """Compile both flavours.  Returns the two paths; raises when a compile fails."""
    if not available():
        raise RuntimeError("reference sources or glib headers not present")
    os.makedirs(OUT_DIR, exist_ok=True)
    srcs = [os.path.join(src_dir(), f + ".c") for f in FILES]
    deps = srcs + [os.path.join(src_dir(), "genhalf.py"), os.path.join(REFERENCE, "include", "framework.h"),
                   os.path.join(REFERENCE, "include", "half.h"), os.path.join(SHIM, "GL", "glew.h"), os.path.abspath(__file__)]
    newest = max(os.path.getmtime(d) for d in deps)
    outs = [path(f) for f in FLAVOURS]
    if not force and all(os.path.exists(o) and os.path.getmtime(o) >= newest for o in outs):
        return outs
    halftab = _halftab()
    inc, cfg, libdir = glib_dirs()
    for name, (_, cc, flags) in FLAVOURS.items():
        cmd = ([cc] + flags + COMMON + ["-I" + os.path.join(REFERENCE, "include"), "-I" + SHIM, "-I" + inc, "-I" + cfg,
                                       "-shared", "-o", path(name)] + srcs + [halftab]
               # -Bsymbolic: libcanvas_hip.so exports the same names globally; the reference must call its own
               + ["-Wl,-Bsymbolic", "-L" + libdir, "-Wl,-rpath," + libdir, "-lglib-2.0", "-lgthread-2.0", "-lm"])
        _run(cmd)
    return outs


if __name__ == "__main__":
    for o in build(force="--force" in sys.argv[1:]):
        print(o)
