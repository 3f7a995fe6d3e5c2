#!/usr/bin/env python3
"""The bits of the score backward: for a fixed list of tiny problems, one line per case -- the case id and the SHA-256 of each
direction's dA bytes.  tests/golden/score_bwd_bits.json holds the output of the build that last changed the arithmetic on purpose;
tests/test_gpu_score_bwd_bits.py recomputes the digests and compares case by case.

    python tools/score_bwd_bits.py                                   # the lines
    python tools/score_bwd_bits.py --out FILE --commit ID            # the JSON file (header: commit, ROCm, device)

The cases are the smallest that reach every path of the backward kernels' shared device parts (csrc/tt_score_bwd_parts.h):
  bf16/...   the seven kernels of bwd_bf16(), picked by D in {20, 64, 100, 256} and TT_OPT_SCORE_BWD_ROWS_MIN in {1, 10^9} as
             tests/_score_forms.bwd_kernel does; square B = 70 (ragged last b tile, two a tiles, the diagonal crossing a tile edge)
             and (Ra, Rb, off) = (70, 210, 70); the rows forms also at B = 130 and 257, either side of their 128- and 256-row
             workgroups; each x {unit, non-unit} x {reciprocals given, NULL}.  The rectangular entry of ops takes neither a unit
             scale nor reciprocals, so the rectangular cases fill tt_score_bwd_dir themselves.
  lq/...     score_bwd_bf16_lq and its x3 variant, same D, B = 70, weights from sampling_bias.log_sampling_probs over a count vector
             with repeated values (D = 100 and 256: the weights loaded behind the S product); bf16 also in the rows form.
  x3/...     bf16x3 operands (D = 256: the single-buffer sweep).
  fp8/...    D in {64, 100, 256}, TT_OPT_FP8_GRAD 1 (rows8) and 0 (rows with fp8 S operands), square B = 130 and 97, and
             (Ra, Rb, off) = (94, 130, 37): diagonals in the second tile of a pair, the last own row's positive at Rb, one past the
             end (rows8's diag_ok epilogue).  ops has no fp8 entry with an offset: these cases fill tt_score_bwd_dir themselves.
  hosted     one eager step at B = 192, H = D = 64 with TT_OPT_FUSE_SCORE_TAIL on (tests/_eager_step.py): d_emb of both towers;
             the step must take one library launch fewer than the same step with the option off, or the digest is refused.
Operands: tests/_score_forms.make_problem, for fp8 plain normal rows L2-normalised with the same seed rule."""
import argparse
import hashlib
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "oracle", ROOT / "tests"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

DEV = "cuda:0"
T = 0.07
DIMS = (20, 64, 100, 256)
ROWS_ALWAYS, ROWS_NEVER, ROWS_MIN_DEFAULT = 1, 1000000000, 32768


def _sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


def _f32(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)


def _padded(t):
    out = torch.ones((t.numel() + 63) // 64 * 64, dtype=t.dtype, device=t.device)
    out[:t.numel()] = t
    return out


def _bf16_cases(ops, L, F, out):
    inv_t = 1.0 / T
    one = torch.ones(1, device=DEV)
    dev = torch.device(DEV)
    for D in DIMS:
        rows_forms = (ROWS_NEVER, ROWS_ALWAYS) if F.padded_d(D) >= 64 else (ROWS_NEVER,)
        for unit in (True, False):
            sn = ops.score_unit_scale(inv_t) if unit else 1.0
            for Ra, Rb, off in ((70, 70, 0), (70, 210, 70), (130, 130, 0), (257, 257, 0)):
                forms = rows_forms if Ra <= 70 else tuple(r for r in rows_forms if r == ROWS_ALWAYS)
                if not forms:
                    continue
                p = F.make_problem(F.Group(Ra, Rb, off, D, T, unit))
                tn, tc = _f32(p.n), _f32(p.c)
                Np, Cp = ops.score_pack2_bf16(tn, tc, sn, 1.0)
                rs, cs, _, _, _, _, inv = ops.score_fwd_bf16(Np, Cp, Rb, D, inv_t, inv_t, True, True, sn, with_inv=True)
                scale = inv_t / (2.0 * Rb)
                if Ra != Rb:                                     # the own rows' images; per-row arrays of the own rows, whole tiles
                    s = slice(off, off + Ra)
                    Npl, Cpl = ops.score_pack2_bf16(tn[s].contiguous(), tc[s].contiguous(), sn, 1.0)
                    own = [_padded(x[s]) for x in (rs, cs, inv[0], inv[1])]
                    full = [_padded(x) for x in (rs, cs, inv[0], inv[1])]
                for rows_min in forms:
                    L.set_option(dev, L.TT_OPT_SCORE_BWD_ROWS_MIN, rows_min)
                    for with_inv in (True, False):
                        if Ra == Rb:
                            dN, dC = ops.score_bwd_bf16(Np, Cp, Rb, D, inv_t, inv_t, rs, cs, one, scale, sn, inv if with_inv else None)
                        else:
                            dN = torch.empty((Ra, D), dtype=torch.float32, device=DEV)
                            dC = torch.empty((Ra, D), dtype=torch.float32, device=DEV)
                            arr = (L.ScoreBwdDir * 2)()
                            ia = (L.ptr(own[2]), L.ptr(own[3]), L.ptr(full[2]), L.ptr(full[3])) if with_inv else (None,) * 4
                            arr[0] = L.ScoreBwdDir(L.ptr(Npl), L.ptr(Cp), Ra, Rb, off, L.ptr(own[0]), L.ptr(full[1]), L.ptr(dN), sn, 1.0, ia[0], ia[3])
                            arr[1] = L.ScoreBwdDir(L.ptr(Cpl), L.ptr(Np), Ra, Rb, off, L.ptr(own[1]), L.ptr(full[0]), L.ptr(dC), sn, sn, ia[1], ia[2])
                            L.check(L.load().tt_score_bwd_bf16(L.ctx(dev), arr, 2, D, inv_t, inv_t, L.ptr(one), scale, L.stream(dev)),
                                    "tt_score_bwd_bf16")
                        form = "rows" if rows_min == ROWS_ALWAYS else "small"
                        out[f"bf16/D{D}/{form}/Ra{Ra}-Rb{Rb}-off{off}/{'unit' if unit else 'nonunit'}/{'inv' if with_inv else 'noinv'}"] = \
                            [_sha(dN), _sha(dC)]


def _lq_x3_cases(ops, L, F, out):
    from jodalrob_twotower_amd.sampling_bias import log_sampling_probs
    inv_t, B = 1.0 / T, 70
    one = torch.ones(1, device=DEV)
    dev = torch.device(DEV)
    lq_n = log_sampling_probs(np.repeat(np.arange(B), 1 + np.arange(B) % 5), B).to(DEV)
    lq_c = log_sampling_probs(np.repeat(np.arange(B), 1 + (np.arange(B) // 2) % 3), B).to(DEV)
    scale = inv_t / (2.0 * B)
    for D in DIMS:
        for unit in (True, False):
            sn = ops.score_unit_scale(inv_t) if unit else 1.0
            u = "unit" if unit else "nonunit"
            p = F.make_problem(F.Group(B, B, 0, D, T, unit))
            tn, tc = _f32(p.n), _f32(p.c)
            for x3 in (False, True):
                Np, Cp = (ops.score_pack2_bf16x3 if x3 else ops.score_pack2_bf16)(tn, tc, sn, 1.0)
                rs, cs, _, _, inv, w, _, _ = ops.score_fwd_sym_lq(Np, Cp, B, D, inv_t, inv_t, lq_n, lq_c, sn, True, x3=x3)
                forms = (ROWS_NEVER, ROWS_ALWAYS) if (not x3 and F.padded_d(D) >= 64) else (ROWS_NEVER,)
                for rows_min in forms:
                    L.set_option(dev, L.TT_OPT_SCORE_BWD_ROWS_MIN, rows_min)
                    dN, dC = ops.score_bwd_bf16_lq(Np, Cp, B, D, inv_t, inv_t, rs, cs, one, scale, w, sn, inv, x3=x3)
                    form = "x3" if x3 else ("rows" if rows_min == ROWS_ALWAYS else "small")
                    out[f"lq/D{D}/{form}/B{B}/{u}"] = [_sha(dN), _sha(dC)]
                L.set_option(dev, L.TT_OPT_SCORE_BWD_ROWS_MIN, ROWS_MIN_DEFAULT)
                if x3:
                    rs, cs, _, _, _, _, inv = ops.score_fwd_bf16(Np, Cp, B, D, inv_t, inv_t, True, True, sn, with_inv=True, x3=True)
                    for with_inv in (True, False):
                        dN, dC = ops.score_bwd_bf16(Np, Cp, B, D, inv_t, inv_t, rs, cs, one, scale, sn, inv if with_inv else None, x3=True)
                        out[f"x3/D{D}/B{B}/{u}/{'inv' if with_inv else 'noinv'}"] = [_sha(dN), _sha(dC)]


def _fp8_cases(ops, L, out):
    inv_t = 1.0 / T
    one = torch.ones(1, device=DEV)
    dev = torch.device(DEV)
    for D in (64, 100, 256):
        for B in (130, 97):
            rng = np.random.default_rng(1000003 * B + 1009 * B + 31 * D)
            n, c = rng.standard_normal((B, D)), rng.standard_normal((B, D))
            tn = _f32(n / np.linalg.norm(n, axis=1, keepdims=True))
            tc = _f32(c / np.linalg.norm(c, axis=1, keepdims=True))
            for unit in (True, False):
                sn = ops.score_unit_scale(inv_t) if unit else 1.0
                Np, Cp = ops.score_pack2_fp8(tn, tc, sn, 1.0)
                rs, cs, _, _, inv, _, _ = ops.score_fwd_sym(Np, Cp, B, D, inv_t, inv_t, sn, True, fp8=True)
                for grad8 in (1, 0):
                    L.set_option(dev, L.TT_OPT_FP8_GRAD, grad8)
                    for with_inv in (True, False):
                        dN, dC = ops.score_bwd_bf16(Np, Cp, B, D, inv_t, inv_t, rs, cs, one, inv_t / (2.0 * B), sn,
                                                    inv if with_inv else None, fp8=True)
                        out[f"fp8/D{D}/{'rows8' if grad8 else 'rows'}/B{B}/{'unit' if unit else 'nonunit'}/{'inv' if with_inv else 'noinv'}"] = \
                            [_sha(dN), _sha(dC)]
                if B != 130:
                    continue
                # the own rows 37 .. 130 of the same problem: their images, their per-row arrays in whole tiles
                Ra, off = 94, 37
                sl = slice(off, off + Ra)
                Npl, Cpl = ops.score_pack2_fp8(tn[sl].contiguous(), tc[sl].contiguous(), sn, 1.0)
                own = [_padded(x[sl]) for x in (rs, cs, inv[0], inv[1])]
                full = [_padded(x) for x in (rs, cs, inv[0], inv[1])]
                for grad8 in (1, 0):
                    L.set_option(dev, L.TT_OPT_FP8_GRAD, grad8)
                    for with_inv in (True, False):
                        dN = torch.empty((Ra, D), dtype=torch.float32, device=DEV)
                        dC = torch.empty((Ra, D), dtype=torch.float32, device=DEV)
                        arr = (L.ScoreBwdDir * 2)()
                        ia = (L.ptr(own[2]), L.ptr(own[3]), L.ptr(full[2]), L.ptr(full[3])) if with_inv else (None,) * 4
                        arr[0] = L.ScoreBwdDir(L.ptr(Npl), L.ptr(Cp), Ra, B, off, L.ptr(own[0]), L.ptr(full[1]), L.ptr(dN), sn, 1.0, ia[0], ia[3])
                        arr[1] = L.ScoreBwdDir(L.ptr(Cpl), L.ptr(Np), Ra, B, off, L.ptr(own[1]), L.ptr(full[0]), L.ptr(dC), sn, sn, ia[1], ia[2])
                        L.check(L.load().tt_score_bwd_fp8(L.ctx(dev), arr, 2, D, inv_t, inv_t, L.ptr(one), inv_t / (2.0 * B), L.stream(dev)),
                                "tt_score_bwd_fp8")
                        out[f"fp8/D{D}/{'rows8' if grad8 else 'rows'}/Ra{Ra}-Rb{B}-off{off}/{'unit' if unit else 'nonunit'}/"
                            f"{'inv' if with_inv else 'noinv'}"] = [_sha(dN), _sha(dC)]


def _hosted_case(tt, out):
    from _eager_step import _batch, _one_step
    schema = json.loads((ROOT / "tests" / "golden" / "schema_real.json").read_text())
    batch, state = _batch(schema, 192, 1092), {}
    _, n_apart, _ = _one_step(tt, schema, state, batch, [128, 64], 64, 0.0, fuse=False)
    got, n_hosted, pending = _one_step(tt, schema, state, batch, [128, 64], 64, 0.0, fuse=True)
    if n_hosted != n_apart - 1 or pending & 4:
        raise RuntimeError(f"the score backward did not run inside the towers' launch: {n_hosted} launches against {n_apart}, pending {pending}")
    out["hosted/B192/H64/D64"] = [_sha(got["d_emb0"]), _sha(got["d_emb1"])]


def digests():
    """{case id: [sha256 of direction 0's dA, of direction 1's]}.  Leaves TT_OPT_SCORE_BWD_ROWS_MIN, TT_OPT_FP8_GRAD and
    TT_OPT_FUSE_SCORE_TAIL at their defaults (32768, 1, 0): the library has no call that reads an option back."""
    import jodalrob_twotower_amd as tt
    from jodalrob_twotower_amd import _lib as L
    from jodalrob_twotower_amd import ops
    import _score_forms as F
    dev = torch.device(DEV)
    out = {}
    try:
        L.set_option(dev, L.TT_OPT_FUSE_SCORE_TAIL, 0)
        _bf16_cases(ops, L, F, out)
        _lq_x3_cases(ops, L, F, out)
        _fp8_cases(ops, L, out)
        L.set_option(dev, L.TT_OPT_SCORE_BWD_ROWS_MIN, ROWS_MIN_DEFAULT)
        _hosted_case(tt, out)
        torch.cuda.synchronize()
    finally:
        L.set_option(dev, L.TT_OPT_SCORE_BWD_ROWS_MIN, ROWS_MIN_DEFAULT)
        L.set_option(dev, L.TT_OPT_FP8_GRAD, 1)
        L.set_option(dev, L.TT_OPT_FUSE_SCORE_TAIL, 0)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="write the JSON file (tests/golden/score_bwd_bits.json) instead of printing the lines")
    ap.add_argument("--commit", default="unknown", help="the commit the library was built from (header of the JSON file)")
    a = ap.parse_args()
    d = digests()
    for k, v in d.items():
        print(k, *v)
    if a.out:
        head = {"commit": a.commit, "rocm": torch.version.hip, "device": torch.cuda.get_device_name(0),
                "note": "digests of the build named here; a change that alters the arithmetic on purpose regenerates this file and says so"}
        Path(a.out).write_text(json.dumps({"header": head, "cases": d}, indent=1) + "\n")
