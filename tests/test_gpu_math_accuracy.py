"""Dense accuracy of the kernels' transcendentals on the device, in all three flavours.

tests/native/math_accuracy_check.hip evaluates sincos_f64 (with and without the 2 pi fold), fold_2pi, sincos_delta,
atan2_pos, angle_of and matrix_to_quat over ~2 x 10^6 points per range (tiny arguments, |x| up to 65536 and 1e15,
the neighbourhoods of k pi / 2 and of the fold switch, the arctangent's reduction switch points, rotations near angle
pi / trace 0 / ties of the diagonal), on the device and on the host from the same source, against long double.
Asserted: every device result is bit-identical to the host's; the errors are within the bounds written beside the
functions in pick_ik_amd/csrc/pik_math.hpp (bound() below); the worst inputs, re-evaluated with mpmath, are within the
same bounds (a guard against a wrong long double reference).  The host half alone runs without a GPU
(tests/test_host_math_cpu.py test_math_accuracy_host_half)."""
import json
import os
import subprocess

import mpmath
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "math_accuracy_check.hip")
HIPCC = "/opt/rocm/bin/hipcc"
# the flags pick_ik_amd/build.py compiles each flavour with
FLAVOURS = {"fast": ["-ffp-contract=on"], "exact_fma": ["-DPIK_STRICT=1", "-DPIK_EXACT_FMA=1", "-ffp-contract=off"],
            "strict": ["-DPIK_STRICT=1", "-ffp-contract=off"]}
N_DEVICE = int(os.environ.get("PIK_MATH_POINTS", "2000000"))

# (function, range) -> ("ulp" | "abs", bound); the same figures stand beside the functions in pik_math.hpp
SINCOS_ULP = 2.0      # |x| <= 65536 + pi: Cody-Waite reduction exact to ~2^-100 relative, kernel ~1 ulp, quadrant exact
SINCOS_FOLD_ABS = 6e-16  # |x| > 65536: the folded argument rounds once or twice (<= 4.5e-16) plus the in-range error


def bound(flavour, fn, rng):
    if fn.startswith("sincos_f64"):
        folded = fn == "sincos_f64<true>" and rng in ("fold_switch_above", "beyond_fold")
        return ("abs", SINCOS_FOLD_ABS) if folded else ("ulp", SINCOS_ULP)
    return {"fold_2pi": ("abs", 4.5e-16),  # two fused steps, each rounding a result of magnitude <= pi + 1: 2 x 2^-52 / 2
            "sincos_delta": ("abs", 2.5e-16),  # inputs from sincos_f64 (<= 1.2e-16 on [-pi, pi]) + ~1e-16 of the step
            "atan2_pos": ("ulp", 2.0 if flavour == "strict" else 3.0),  # fdlibm's 4-way reduction / the 2-step one
            "angle_of": ("ulp", 4.0),  # atan2_pos's error + the rounded norm of the vector part, doubled exactly
            "matrix_to_quat": ("abs", 5e-16),  # the root of a sum >= 1 of three rounded terms, one product per component
            }[fn]


def build(flavour, device=True):
    tag = "" if device else "_host"
    exe = os.path.join(ROOT, "tests", "native", f"math_accuracy_check_{flavour}{tag}")
    deps = [SRC] + [os.path.join(ROOT, "pick_ik_amd", "csrc", f) for f in ("pik_math.hpp", "pik_host.hpp")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(map(os.path.getmtime, deps)):
        if device:
            # (-Xarch_host -mfma: the host pass contracts a * b + c as the device does -- the x86-64 baseline has no
            # fused multiply-add, and an uncontracted host would differ from the device, not the device from itself)
            cmd = [HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-Xarch_host", "-mfma", *FLAVOURS[flavour], SRC,
                   "-o", exe]
        else:  # the host half: g++ with the flags tests/test_host_math_cpu.py builds the same headers with
            flags = [] if flavour == "fast" else FLAVOURS[flavour]
            cmd = ["g++", "-std=c++17", "-O2", "-mfma", *flags, "-x", "c++", SRC, "-o", exe]
        subprocess.run(cmd, check=True)
    return exe


def _mp_error(fn, xs, out):
    """(ulp error, abs error) of a result against mpmath at 128 bits"""
    M = mpmath.MPContext()
    M.prec = 128
    x = [M.mpf(v) for v in xs]
    if fn.startswith("sincos_f64"):
        refs = [M.sin(x[0]), M.cos(x[0])]
    elif fn == "atan2_pos":
        refs = [M.atan2(x[0], x[1])]
    elif fn == "angle_of":
        refs = [2 * M.atan2(M.sqrt(x[1] ** 2 + x[2] ** 2 + x[3] ** 2), abs(x[0]))]
    elif fn == "fold_2pi":
        k = M.mpf(round(xs[0] * 0.15915494309189535))  # (the kernel's k: rint of the rounded product)
        refs = [x[0] - 2 * M.pi * k]
    else:
        return None
    eu = ea = 0.0
    for o, r in zip(out, refs):
        d = abs(M.mpf(o) - r)
        ulp = 2.0 ** (int(M.floor(M.log(abs(r), 2))) - 52) if r != 0 else 2.0 ** -1074
        eu, ea = max(eu, float(d / ulp)), max(ea, float(d))
    return eu, ea


def check(flavour, lines, device):
    """assert the bounds on the JSON lines of one run; returns {(fn, range): (max_ulp, max_abs)}"""
    seen = {}
    if device:  # (every range's count first: one failure should not hide the others)
        bad = [(d["fn"], d["range"], d["device_mismatch"]) for d in lines if d["device_mismatch"] != 0]
        assert not bad, (flavour, "device results that differ from the host's", bad)
    for d in lines:
        fn, rng = d["fn"], d["range"]
        if rng == "special":
            vals = [[float.fromhex(v) for v in row] for row in d["values"]]
            for x, s, c in vals:
                if x == 0.0:  # sin(+-0) = 0 (the reduction's x - 0 pi/2 turns -0 into +0: no use reads the sign), cos = 1
                    assert s == 0.0 and c == 1.0, (flavour, fn, x, s, c)
                else:  # +-inf, NaN: NaN out (and the call returned)
                    assert s != s and c != c, (flavour, fn, x, s, c)
            continue
        assert d["nonfinite"] == 0, (flavour, fn, rng, d)
        metric, b = bound(flavour, fn, rng)
        val = d["max_ulp"] if metric == "ulp" else d["max_abs"]
        assert val <= b, (flavour, fn, rng, metric, val, b, d)
        for key in ("worst_ulp", "worst_abs"):  # the worst inputs against mpmath
            xs = [float.fromhex(v) for v in d[key + "_in"]]
            out = [float.fromhex(v) for v in d[key + "_out"]]
            e = _mp_error(fn, xs, out)
            if e is not None:
                assert (e[0] if metric == "ulp" else e[1]) <= b, (flavour, fn, rng, key, xs, out, e, b)
        seen[(fn, rng)] = (d["max_ulp"], d["max_abs"])
    return seen


def run(exe, n, timeout):
    r = subprocess.run([exe, str(n)], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return [json.loads(ln) for ln in r.stdout.strip().splitlines()]


@pytest.mark.gpu
def test_device_math_accuracy_all_flavours():
    """the three flavours' binaries run side by side (one process each; the host reference dominates the time)"""
    exes = {f: build(f) for f in FLAVOURS}
    procs = {f: subprocess.Popen([exe, str(N_DEVICE)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for f, exe in exes.items()}
    outs = {}
    try:
        for f, p in procs.items():
            so, se = p.communicate(timeout=500)
            assert p.returncode == 0, (f, p.returncode, se[-2000:])
            outs[f] = [json.loads(ln) for ln in so.strip().splitlines()]
    finally:
        for p in procs.values():
            if p.poll() is None:
                p.kill()
    for f, lines in outs.items():
        seen = check(f, lines, device=True)
        assert len(seen) == 24, (f, sorted(seen))
        for (fn, rng), (u, a) in sorted(seen.items()):
            print(f"{f:9s} {fn:18s} {rng:22s} max {u:8.4g} ulp  {a:.3g} abs")
