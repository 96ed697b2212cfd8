"""Build libpss.so (HIP kernels + C ABI) in-tree for gfx950 with hipcc.

    python -m pyspecsdr_amd.build        # or: from pyspecsdr_amd.build import build; build()

hipcc cross-compiles gfx950 without a GPU present.  The library lands at pyspecsdr_amd/libpss.so (git-ignored,
but shipped to the GPU box with the working tree).
"""
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "libpss.so")
BUILD = os.path.join(HERE, "_build")

ARCH = "gfx950"
COMMON = ["--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "-Wno-unused-value", "-Wno-unused-result"]
# pss_demod.hip carries the bit-exactness contract: no implicit fused multiply-adds.
DEMOD_FLAGS = ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt", "-mllvm", "-instcombine-max-copied-from-constant-users=4000"]
UNITS = [
    ("pss_fft.hip", ["-fhip-fp32-correctly-rounded-divide-sqrt"]),   # the scanner rows use NumPy's float32 abs (IEEE sqrt / divide)
    # -instcombine-max-copied-from-constant-users: the FIR taps are a by-value kernel argument read at many (dynamic) offsets; past
    # LLVM's default of 300 users instcombine no longer forwards the reads to the kernarg segment and the whole table is copied to
    # scratch at kernel entry (measured: 412 spilled VGPRs in k_nfm_fwd instead of 3)
    ("pss_demod.hip", DEMOD_FLAGS),
    ("pss_pipeline.hip", DEMOD_FLAGS),   # the batched loop iterations around the demodulator: host code and one conversion kernel
    ("pss_squelch.hip", ["-ffp-contract=off"]),   # NumPy's summation tree and np.max, bit for bit: no fused multiply-adds either
    ("pss_ingest.hip", ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"]),   # int16 codes / scale: one IEEE float32 division
    ("pss_decode_dev.hip", ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"]),   # the decoders' back halves for batches: observation-order sums, one float32 division
    ("pss_mono.hip", ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"]),   # decode_mono and lfilter: NumPy's / SciPy's float32 and float64 operations one by one
    ("pss_ddc.hip", ["-ffp-contract=off"]),   # the down-converter: every fused multiply-add is written as fma, nothing else is fused
    ("pss_pfb.hip", ["-ffp-contract=off"]),   # the polyphase channeliser: the same rule
    ("pss_bank.hip", ["-ffp-contract=off"]),   # the channeliser for 2^a 3^b 5^c grids: the same rule
    ("pss_resample.hip", ["-ffp-contract=off"]),   # the rational resampler: SciPy's upfirdn, one multiply and one add per tap
    ("pss_welch.hip", ["-ffp-contract=off"]),   # the capture survey: every fused multiply-add is written as fma
    ("pss_rds.hip", ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"]),   # the RDS receiver: NumPy's float32 arctan2, then fma chains written as fma
    ("pss_adsb.hip", ["-ffp-contract=off"]),   # the Mode S receiver: float32 products and sums one by one, strict comparisons
    ("pss_ais.hip", ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"]),   # the AIS receiver: NumPy's float32 arctan2, one fma chain, strict comparisons
    ("pss_pocsag.hip", ["-ffp-contract=off"]),   # the POCSAG receiver: float32 sums one by one, strict comparisons, integer BCH arithmetic
    ("pss_flex.hip", ["-ffp-contract=off"]),   # the FLEX receiver: float32 sums one by one, strict comparisons, pss_pocsag.h's BCH arithmetic
    ("pss_apt.hip", ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"]),   # the APT receiver: NumPy's float32 arctan2, fma chains, float32 sums and divisions one by one
    ("pss_ook.hip", ["-ffp-contract=off"]),   # the OOK receiver: float32 products and sums one by one, float64 sums in a stated order, integer slicers
    ("pss_packet.hip", ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"]),   # the packet-radio receiver: NumPy's float32 arctan2, four fma chains, float64 products and one division, integer clock tracking
    ("pss_api.cpp", ["-x", "hip"]),
    ("pss_stream.cpp", ["-x", "hip"]),                        # host only: the streamed captures' chunk loop
    ("pss_design.cpp", ["-x", "hip", "-ffp-contract=off"]),
    ("pss_decode.cpp", ["-x", "hip", "-ffp-contract=off"]),   # host only: the decoders' per-message halves
    ("pss_comm.cpp", ["-x", "hip"]),                          # host only: the exchange steps over RCCL (dlopen, no link dependency)
]


def hipcc():
    for c in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found (need ROCm; this package has no CPU fallback)")


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False):
    os.makedirs(BUILD, exist_ok=True)
    cc = hipcc()
    headers = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    headers.append(os.path.join(os.path.dirname(HERE), "include", "pss.h"))
    headers.append(os.path.abspath(__file__))
    objs, running = [], []
    for src, extra in UNITS:   # the translation units compile side by side (the two large .hip files take ~30 s each)
        s = os.path.join(CSRC, src)
        o = os.path.join(BUILD, src.rsplit(".", 1)[0] + ".o")
        objs.append(o)
        if force or _stale(o, [s] + headers):
            cmd = [cc] + COMMON + extra + ["-c", s, "-o", o]
            if verbose:
                print(" ".join(cmd), flush=True)
            running.append((cmd, subprocess.Popen(cmd)))
    for cmd, proc in running:
        if proc.wait() != 0:
            raise subprocess.CalledProcessError(proc.returncode, cmd)
    if force or _stale(OUT, objs):
        cmd = [cc, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-Wl,--strip-all", "-o", OUT] + objs + ["-ldl"]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
    return OUT


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
