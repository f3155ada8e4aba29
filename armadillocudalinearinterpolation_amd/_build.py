"""In-tree build of libmi355interp.so (hand-written HIP, gfx950 only)."""
import glob
import os
import shutil
import subprocess

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
REPO_ROOT = os.path.dirname(PKG_DIR)
CSRC = os.path.join(PKG_DIR, "csrc")
LIB_PATH = os.path.join(PKG_DIR, "libmi355interp.so")

# -ffp-contract=off: the fp64/fp32 blends must round every product and sum
# separately (bit parity with oracle/); correctly rounded fp32 div for Restrict.
HIPCC_FLAGS = [
    "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
    "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt",
    "-Wall", "-Wno-unused-value",
]
# mi_edm.hip without the SLP vectoriser: it pairs the firing test's independent fp32 operations into v_pk_*_f32, and on
# gfx950 a packed fp32 instruction takes more issue time than the two it replaces (same bits either way; measured
# 116.4 -> 113.6 ms at N = 1024, 45.2 -> 43.0 ms at N = 512, profiles/r04_edm_evolve_steps.log).
# mi_interp1.hip exports its dispatcher and its launch counter under a second name: the names themselves are defined
# in mi_sweep_phase.hip, which forwards to these (the files of the interp1 family stay as they are, byte for byte).
PER_SOURCE_FLAGS = {
    "mi_edm.hip": ["-fno-slp-vectorize"],
    "mi_interp1.hip": ["-Dmi_interp1_f64_dev_v2=mi_interp1_f64_dev_v2_base",
                       "-Dmi_debug_sweep_ds_launches=mi_debug_sweep_ds_launches_base"],
}


def sources():
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")))


def _deps():
    return sources() + glob.glob(os.path.join(CSRC, "*.hpp")) + glob.glob(os.path.join(REPO_ROOT, "include", "*.h"))


def source_hash(family=None):
    """sha256 over the device / ABI sources the library is built from (sorted paths, contents only): what a committed
    profile is stamped with, so that bench.py can tell whether a measured traffic figure belongs to the running build.
    family="interp1" / "interp2" / "edm": only the sources that kernel family is compiled from (mi_<family>*, mi_common.hpp,
    mi_ctx.hip), so that work on another kernel family -- or a comment in the ABI header -- does not orphan a traffic profile."""
    import hashlib
    h = hashlib.sha256()
    for p in sorted(_deps()):
        b = os.path.basename(p)
        if family and not (b.startswith("mi_" + family) or b in ("mi_common.hpp", "mi_ctx.hip")):
            continue
        h.update(b.encode())
        h.update(open(p, "rb").read())
    return h.hexdigest()


def is_stale():
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    return any(os.path.getmtime(p) > t for p in _deps())


def build_lib(force=False, verbose=False):
    """Compile csrc/*.hip -> libmi355interp.so with hipcc (cross-compiles without a GPU): one object per translation
    unit, compiled in parallel (csrc/build/, git-ignored), then one link."""
    if not force and not is_stale():
        return LIB_PATH
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        raise RuntimeError("hipcc not found: libmi355interp.so cannot be built (there is no CPU fallback)")
    # One builder at a time (bench.py --gpus N starts N ranks that all import the package: with a stale library they would
    # compile into the same object files at once and one could link what another is still writing).  The lock is held for
    # the whole build; whoever waited finds the library fresh and returns.
    import fcntl
    os.makedirs(os.path.join(CSRC, "build"), exist_ok=True)
    with open(os.path.join(CSRC, "build", ".lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not force and not is_stale():
            return LIB_PATH
        return _build_locked(hipcc, force, verbose)


def _build_locked(hipcc, force, verbose):
    from concurrent.futures import ThreadPoolExecutor
    extra = os.environ.get("MI_EXTRA_HIPCC_FLAGS", "").split()
    flags = [f for f in HIPCC_FLAGS if f != "-shared"] + extra + ["-I", os.path.join(REPO_ROOT, "include"), "-I", CSRC]
    objdir = os.path.join(CSRC, "build")
    os.makedirs(objdir, exist_ok=True)
    hdr_t = max(os.path.getmtime(p) for p in _deps() if not p.endswith(".hip"))
    stamp = " ".join(flags) + " " + repr(sorted(PER_SOURCE_FLAGS.items()))
    stamp_path = os.path.join(objdir, "flags.txt")
    same_flags = os.path.exists(stamp_path) and open(stamp_path).read() == stamp

    def compile_one(src):
        obj = os.path.join(objdir, os.path.basename(src)[:-4] + ".o")
        if (not force and same_flags and os.path.exists(obj) and os.path.getmtime(obj) > os.path.getmtime(src)
                and os.path.getmtime(obj) > hdr_t):
            return obj
        cmd = [hipcc] + flags + PER_SOURCE_FLAGS.get(os.path.basename(src), []) + ["-c", src, "-o", obj]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
        return obj

    with ThreadPoolExecutor(max_workers=min(6, os.cpu_count() or 1)) as ex:
        objs = list(ex.map(compile_one, sources()))
    open(stamp_path, "w").write(stamp)
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB_PATH + ".tmp"] + objs
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    os.replace(LIB_PATH + ".tmp", LIB_PATH)
    return LIB_PATH


if __name__ == "__main__":
    print(build_lib(force=True, verbose=True))
