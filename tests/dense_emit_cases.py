"""What the tests of the register-resident scans' emit and sample pass share (tests/test_gpu_dense_emit.py
and its host companion): the workspace carve of a packed f16 batch, make_plan's sample, the row order of
the fragment-major float16 copy.  Python replicas of csrc/dense.hip / dense_common.hpp, checked against
the library by tests/test_dense_emit_host.py."""
import math
import os

import numpy as np

CAND_CAP = 16384          # dense_common.hpp
QREG_MAX_SEG = 1024
SAMPLE_TOP = 4
SEL_BIG_BAND = 1024
CAND_BYTES = 8            # struct Cand {float score; uint32_t doc;}
F32_U = 2.0 ** -24

# make_plan's knobs, read the way dense_knobs() reads them
KS = int(os.environ.get("THR_DENSE_KS") or 32)
KS = KS if 4 <= KS <= 64 else 32
AIM_1M = float(os.environ.get("THR_DENSE_AIM") or 1448.0)
AIM_1M = AIM_1M if AIM_1M >= 64.0 else 1448.0


def carve(qtile, nq, dim):
    """{name: (byte offset, bytes)} of make_plan's workspace for a packed batch (Arena: every piece
    rounded up to 256 bytes), and the total."""
    ntiles = (nq + qtile - 1) // qtile
    qpad = ntiles * qtile
    pieces = [("tau", 4 * qpad), ("qerr", 4 * qpad), ("cnt", 4 * qpad * QREG_MAX_SEG), ("tcnt", 4 * ntiles),
              ("cand", CAND_BYTES * qpad * CAND_CAP), ("tlist", CAND_BYTES * ntiles),
              ("sample", 4 * qpad * QREG_MAX_SEG * SAMPLE_TOP), ("qfrag", 2 * qpad * dim),
              ("sel_rows", 4 * qpad * SEL_BIG_BAND), ("sel_meta", 4 * 4 * qpad)]
    out, total = {}, 0
    for name, nbytes in pieces:
        out[name] = (total, nbytes)
        total += (nbytes + 255) & ~255
    return out, total, qpad


def plan(n, kprime):
    """make_plan's sample of a packed batch -> (stride in 32-row groups, groups sampled): sample group i
    is row group i * stride."""
    groups = (n + 31) // 32
    ks = min(kprime, KS)
    aim = AIM_1M * math.sqrt(n / 1.0e6)
    aim = min(max(aim, min(8.0 * kprime, 4096.0)), 4096.0)
    target = max(min(int(n * ks / aim), 1 << 20), 4 * ks)
    sg = min((target + 31) // 32, groups)
    return groups // sg, sg


def unpack_copy16(docs16, dim, shape=16):
    """The fragment-major float16 copy (quantize_f16_norm) -> row-major [rows padded to 32, dim].
    16x16x32 shape: piece 2 k32 + ra of a 32-row tile = rows [16 ra, +16) x dims [32 k32, +32), lane
    (r & 15) + 16 g, 8 halves per lane.  32x32x16: piece s = 32 rows x dims [16 s, +16), lane r + 32 hh."""
    if shape == 32:
        a = np.asarray(docs16).reshape(-1, dim // 16, 2, 32, 8)     # tile, s, hh, r, e
        return a.transpose(0, 3, 1, 2, 4).reshape(-1, dim)
    a = np.asarray(docs16).reshape(-1, dim // 32, 2, 4, 16, 8)      # tile, k32, ra, g, r & 15, e
    return a.transpose(0, 2, 4, 1, 3, 5).reshape(-1, dim)


def segment_of_row(r, shape=16):
    """The lane group (candidate / sample segment within a row slice) that holds row r of a 32-row tile.
    QAcc<16> / QAcc<48>: register 4 (..) + j is row 16 ra + 4 g + j; QAcc<32>: register x is row
    (x & 3) + 8 (x >> 2) + 4 h."""
    return (r // 4) % 2 if shape == 32 else (r % 16) // 4


def scan_slack(q):
    """fp32 accumulation bound of the scan (scan_eps, dense_common.hpp): (dim + 16) 2^-24 ||q|| ||d||,
    ||d|| = 1 -- how far the kernel's float32 sum of the float16 products may lie from their float64
    sum.  From the number format alone."""
    return (len(q) + 16) * F32_U * float(np.linalg.norm(q.astype(np.float64))) * (1 + 2.0 ** -10)
