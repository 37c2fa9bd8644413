"""A plain model of the range tables of the adaptive compaction passes, written from DESIGN.md section 4
("Persistent waves + compaction passes", "Two register budgets", "Latency-greedy or efficiency-greedy") and section 9
-- it does not call the library.

A memetic call on one tip frame with one species offers every pass these kernel variants, widest first
(ids: pick_ik_amd.Solver.VARIANT_LANES): 16 / 8 / 4 / 2 lanes per elite (5 / 4 / 3 / 2) where a problem's
gs * lanes fit a wavefront, the one-lane kernel compiled for one wavefront per SIMD (1) and, for chains of up to nine
variables, for two (7).  A variant serves the survivor counts in (lo, hi]:

  * more than one lane per elite: hi = the problems that get a wavefront each in one round, SIMDs * (64 / (gs * lanes));
  * one lane, one per SIMD: hi = occ2_from * 64 / gs - 1, occ2_from (first-pass wavefronts from which the second
    wavefront per SIMD pays) = 9/8 of the SIMD count with the chip to the call, 5/8 with other calls on it; an explicit
    option two_per_simd > 1 is that figure in both regimes; without the two-per-SIMD variant it takes everything;
  * one lane, two per SIMD: everything above.

lo is the hi of the entry in front; a range that comes out empty is never chosen.  The throughput regime has the
one-lane variants only.  The router of a pass takes the throughput table when the other slots hold at least
`threshold` problems (default: half of the problems that give every SIMD a one-lane wavefront) and hands the pass to
the entry whose range holds the survivor count; a pass without survivors runs nothing (variant id 0)."""
import numpy as np

WAVE = 64
MAX_COUNT = 0xFFFFFFFF
WIDE = ((16, 5), (8, 4), (4, 3), (2, 2))  # (lanes per elite, variant id), widest first


def pow2ceil(n):
    return 1 << max(int(n) - 1, 0).bit_length()


def allowed_widths(gs, general_dh_step=False):
    """the widths above one lane a call may use: a problem's gs * v lanes fit a wavefront; the fast flavour's
    cooperative descent (8 / 16 lanes) does not exist for a chain with a general Denavit-Hartenberg step"""
    return {v for v, _ in WIDE if gs * v <= WAVE and not (general_dh_step and v >= 8)}


def variants(gs, D, widths, two_per_simd=None):
    """(variant id, lanes per elite) of every candidate, widest first; two_per_simd: None = the library's default,
    else the option's value (0: never the two-per-SIMD variant)"""
    out = [(vid, v) for v, vid in WIDE if v in widths]
    assert all(gs * v <= WAVE for _, v in out), (gs, widths)
    out.append((1, 1))
    if D <= 9 and (two_per_simd is None or int(two_per_simd) != 0):
        out.append((7, 1))
    return out


def table(simds, gs, D, widths, two_per_simd=None, throughput=False):
    """the range table of one regime: [(variant id, lo, hi)], the variant chosen for lo < survivors <= hi"""
    var = variants(gs, D, widths, two_per_simd)
    explicit = two_per_simd is not None and int(two_per_simd) > 1
    occ2_from = int(two_per_simd) if explicit else simds * (5 if throughput else 9) // 8
    out, lo = [], 0
    for i, (vid, lanes) in enumerate(var):
        if throughput and lanes > 1:
            continue
        if lanes > 1:
            hi = simds * (WAVE // (gs * lanes))
        elif vid == 7 or i == len(var) - 1:
            hi = MAX_COUNT
        else:
            hi = occ2_from * WAVE // gs - 1
        hi = min(max(hi, lo), MAX_COUNT)
        out.append((vid, lo, hi))
        lo = hi
    return out


def pick(tab, n):
    """the variant id a table gives n problems (0: none)"""
    for vid, lo, hi in tab:
        if lo < n <= hi:
            return vid
    return 0


def default_threshold(simds, gs):
    return simds * WAVE // gs // 2


class Model:
    def __init__(self, simds, elites, D, widths=None, two_per_simd=None, general_dh_step=False):
        self.simds, self.gs, self.D = int(simds), pow2ceil(elites), int(D)
        self.general_dh_step = bool(general_dh_step)
        self.widths = allowed_widths(self.gs, general_dh_step) if widths is None else set(widths)
        self.latency = table(simds, self.gs, D, self.widths, two_per_simd, False)
        self.throughput = table(simds, self.gs, D, self.widths, two_per_simd, True)
        self.threshold = default_threshold(simds, self.gs)

    def widest(self):
        return max(self.widths | {1})

    def route(self, survivors, others, threshold=None):
        """the router's decision for a pass: the variant id"""
        if survivors == 0:
            return 0
        t = self.threshold if threshold is None else threshold
        return pick(self.throughput if others >= t else self.latency, survivors)

    def host(self, B, throughput=False):
        """the host's choice for pass 0, whose size it knows"""
        return pick(self.throughput if throughput else self.latency, B)

    def check_record(self, rec, B, load, threshold=None, host_throughput=False):
        """a routed call's record [(survivors, others' load, variant id)] under a constant published load: every
        entry is this model's decision; returns the variant ids"""
        assert rec is not None and rec[0][0] == B, (rec, B)
        want = [(n, load, self.host(B, host_throughput) if k == 0 else self.route(n, load, threshold))
                for k, (n, _, _) in enumerate(rec)]
        assert rec == want, f"record {rec}\nmodel  {want}"
        assert all(rec[k][0] >= rec[k + 1][0] for k in range(len(rec) - 1)), rec
        return [v for _, _, v in rec]


def general_step_pairs(chain):
    """consecutive joint axes of a serial chain that are nearly but not exactly parallel (the squared sine of their
    angle inside (1e-30, 1e-3), pik_host.hpp build_dh): those pairs take a general constant step in the fast flavour.
    Returns (pairs inside the window, pairs within 1 % of one of its ends -- too close for this double
    precision restatement to call)"""
    from pick_ik_amd import robots

    def rot(rpy):
        r, p, y = rpy
        cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
        return np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                         [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                         [-sp, cp * sr, cp * cr]])

    R, Z = np.eye(3), []
    for j in range(chain.dof):
        jt = int(chain.joint_type[j])
        planar = jt in (robots.PLANAR_X, robots.PLANAR_Y, robots.PLANAR_THETA)
        if planar:  # (x, y, theta of the joint's frame; the first variable carries the origin)
            axis = np.eye(3)[jt - robots.PLANAR_X]
        else:
            axis = np.asarray(chain.axis[j], float) / np.linalg.norm(chain.axis[j])
        if not planar or jt == robots.PLANAR_X:
            R = R @ rot(chain.origin_xyz_rpy[j][3:])
        Z.append(R @ axis)
    inside, close = [], []
    for j in range(chain.dof - 1):
        w = np.cross(Z[j], Z[j + 1])
        sw2 = float(w @ w)
        if 1e-30 < sw2 < 1e-3:
            inside.append(j)
        if 0.99e-30 < sw2 < 1.01e-30 or 0.99e-3 < sw2 < 1.01e-3:
            close.append(j)
    return inside, close
