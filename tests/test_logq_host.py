"""Host-side tests of the logQ sampling-bias correction: the C entries declared, bound and exported, the new struct's layout,
sampling_bias.log_sampling_probs against a numpy bincount, and the refusals of what the correction does not cover (fp8, the
dense loss path, the sharded task, the unrolled / segmented steps, bad log q shapes and dtypes) -- before any device call."""
import ctypes
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT
from jodalrob_twotower_amd import _lib

LQ_SYMBOLS = ("tt_score_fwd_sym_bf16_lq", "tt_score_fwd_sym_bf16x3_lq", "tt_score_bwd_bf16_lq", "tt_score_bwd_bf16x3_lq",
              "tt_score_dir_fwd_lq", "tt_score_dir_bwd_lq", "tt_score_loss_finish_lq")


def test_lq_entries_declared_bound_exported():
    header = (ROOT / "include" / "twotower.h").read_text()
    declared = set(re.findall(r"\b(tt_\w+_lq)\s*\(", header))
    assert declared == set(LQ_SYMBOLS)
    lib = _lib.load()
    for name in LQ_SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    sig = _lib.SIGNATURES
    # each is the plain entry plus the log-probability arrays (and, for the symmetric forward, the weights it leaves)
    assert sig["tt_score_fwd_sym_bf16_lq"][1] == sig["tt_score_fwd_sym_bf16"][1][:9] + [_lib.vp] * 2 + sig["tt_score_fwd_sym_bf16"][1][9:13] \
        + [_lib.vp] * 2 + sig["tt_score_fwd_sym_bf16"][1][13:]
    assert sig["tt_score_fwd_sym_bf16x3_lq"][1] == sig["tt_score_fwd_sym_bf16_lq"][1]
    plain = sig["tt_score_bwd_bf16"][1]
    assert sig["tt_score_bwd_bf16_lq"][1] == plain[:2] + [ctypes.POINTER(_lib.ScoreBwdLq)] + plain[2:]
    assert sig["tt_score_bwd_bf16x3_lq"][1] == sig["tt_score_bwd_bf16_lq"][1]
    assert sig["tt_score_dir_fwd_lq"][1] == sig["tt_score_dir_fwd"][1][:9] + [_lib.vp] + sig["tt_score_dir_fwd"][1][9:]
    assert sig["tt_score_dir_bwd_lq"][1] == sig["tt_score_dir_bwd"][1][:9] + [_lib.vp] * 2 + sig["tt_score_dir_bwd"][1][9:]
    assert sig["tt_score_loss_finish_lq"][1] == sig["tt_score_loss_finish"][1][:3] + [_lib.vp] * 2 + sig["tt_score_loss_finish"][1][3:]
    assert lib.tt_abi_version() == 2


def test_lq_struct_matches_c_layout(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "twotower.h"\nint main(){printf("%zu %zu %zu\\n", sizeof(tt_score_bwd_lq),'
                   'sizeof(tt_score_bwd_dir), sizeof(tt_score_fwd_dir));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    sizes = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    assert sizes == [ctypes.sizeof(_lib.ScoreBwdLq), ctypes.sizeof(_lib.ScoreBwdDir), ctypes.sizeof(_lib.ScoreFwdDir)]


def test_log_sampling_probs_matches_bincount():
    from jodalrob_twotower_amd.sampling_bias import log_sampling_probs
    rng = np.random.default_rng(3)
    idx = np.minimum(rng.zipf(1.3, 5000) - 1, 99)
    idx[idx == 7] = 8                                        # entity 7 has no pair
    lq = log_sampling_probs(torch.from_numpy(idx), 120)
    assert lq.dtype == torch.float32 and lq.shape == (120,)
    ref = np.log(np.maximum(np.bincount(idx, minlength=120), 1) / idx.size)
    assert np.allclose(lq.numpy(), ref, rtol=1e-6, atol=0)
    assert lq[7].item() == pytest.approx(np.log(1 / 5000), rel=1e-6) and lq[119].item() == lq[7].item()
    assert np.allclose(log_sampling_probs(idx, 120).numpy(), lq.numpy())            # numpy input
    with pytest.raises(ValueError):
        log_sampling_probs(np.array([0, 5]), 5)
    with pytest.raises(ValueError):
        log_sampling_probs(np.array([], dtype=np.int64), 5)
    with pytest.raises(TypeError):
        log_sampling_probs(np.array([0.5]), 5)


def _fake_task(score_dtype="bf16", dense=False):
    return SimpleNamespace(score_dtype=score_dtype, _dense_loss=dense, _refused=frozenset())


def _side(B, lq):
    d = {"dense": torch.zeros(B, 3)}
    if lq is not None:
        d["log_q"] = lq
    return d


def test_task_refuses_log_q_it_does_not_cover():
    from jodalrob_twotower_amd.two_tower_train_task import TwoTowerTrainTask
    from jodalrob_twotower_amd.distributed import DistributedTwoTowerTrainTask
    B = 8
    lq = torch.zeros(B)
    def f(task, notice, company, B):
        return TwoTowerTrainTask._batch_terms(task, {"notice": notice, "company": company}, B).lq
    assert f(_fake_task(), _side(B, None), _side(B, None), B) is None
    with pytest.raises(ValueError, match="fp8"):
        f(_fake_task("fp8"), _side(B, lq), _side(B, None), B)
    with pytest.raises(ValueError, match="dense loss"):
        f(_fake_task(dense=True), _side(B, None), _side(B, lq), B)
    with pytest.raises(ValueError, match="shape"):
        f(_fake_task(), _side(B, torch.zeros(B + 1)), _side(B, None), B)
    with pytest.raises(ValueError, match="float32"):
        f(_fake_task(), _side(B, torch.zeros(B, dtype=torch.float64)), _side(B, None), B)
    n, c = f(_fake_task("fp32"), _side(B, None), _side(B, lq + 1), B)   # a missing side counts as zeros
    assert torch.equal(n, torch.zeros(B)) and torch.equal(c, lq + 1)
    with pytest.raises(NotImplementedError, match="sharded"):
        DistributedTwoTowerTrainTask._score_ce(None, None, None, 1.0, False, log_q=(lq, lq))


def test_steps_declare_log_q_support():
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    from jodalrob_twotower_amd.segmented import SegmentedTrainStep
    from jodalrob_twotower_amd.unrolled import UnrolledTrainStep
    assert "log_q" in GraphedTrainStep._accepts and "log_q" not in UnrolledTrainStep._accepts and "log_q" not in SegmentedTrainStep._accepts


class _FakeStore:
    def __init__(self, n):
        self.n, self.device = n, torch.device("cpu")

    def __len__(self):
        return self.n


def _loader(log_q=None, n_pairs=10, batch=4):
    from jodalrob_twotower_amd.data_loader import DevicePairLoader
    pairs = np.stack([np.arange(n_pairs) % 5, np.arange(n_pairs) % 3], axis=1)
    return DevicePairLoader(_FakeStore(5), _FakeStore(3), pairs, batch, shuffle=False, log_q=log_q)


def test_loader_validates_log_q():
    ok = (torch.zeros(5), torch.zeros(3))
    assert _loader(ok).log_q is not None and _loader().log_q is None
    for bad in ((torch.zeros(4), torch.zeros(3)), (torch.zeros(5), torch.zeros(3, dtype=torch.float64)), (torch.zeros(5, 1), torch.zeros(3)),
                (torch.zeros(5),), torch.zeros(5), ([0.0] * 5, torch.zeros(3))):
        with pytest.raises(ValueError):
            _loader(bad)
    ld = _loader()
    with pytest.raises(ValueError):
        ld.set_log_q((torch.zeros(5), torch.zeros(2)))
    ld.set_log_q(ok)
    assert ld.log_q is not None
    ld.set_log_q(None)
    assert ld.log_q is None


def test_loader_epoch_log_q_layout():
    """[n_batches, 2, Bp]: batch k's notice / company log q at [k, 0 / 1, :m], Bp = batch rounded up to 4 (aligned slices)."""
    lqn, lqc = torch.arange(5, dtype=torch.float32) - 10, torch.arange(3, dtype=torch.float32) - 20
    ld = _loader((lqn, lqc), n_pairs=10, batch=3)
    arr = ld.epoch_log_q(None)
    assert arr.shape == (4, 2, 4)
    pairs = ld.pairs
    for k, lo in enumerate(range(0, 10, 3)):
        m = min(3, 10 - lo)
        assert torch.equal(arr[k, 0, :m], lqn[pairs[lo:lo + m, 0]]) and torch.equal(arr[k, 1, :m], lqc[pairs[lo:lo + m, 1]])
        assert arr[k, 0, :m].data_ptr() % 16 == arr.data_ptr() % 16


def test_unrolled_and_segmented_steps_raise_on_log_q():
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    from jodalrob_twotower_amd.segmented import SegmentedTrainStep
    from jodalrob_twotower_amd.unrolled import UnrolledTrainStep
    ex = {"notice": {"dense": torch.zeros(4, 2), "log_q": torch.zeros(4)}, "company": {"dense": torch.zeros(4, 2)}}
    with pytest.raises(NotImplementedError, match="UnrolledTrainStep"):
        UnrolledTrainStep(None, None, ex, unroll=2)
    with pytest.raises(NotImplementedError, match="SegmentedTrainStep"):
        SegmentedTrainStep(None, None, ex)
    with pytest.raises(NotImplementedError, match="sharded"):
        GraphedTrainStep(SimpleNamespace(exchange=object()), None, ex)
    # the loader's fast path with an unrolled step
    ld = _loader((torch.zeros(5), torch.zeros(3)))
    with pytest.raises(NotImplementedError, match="unrolled"):
        next(ld.step_batches(SimpleNamespace(unroll=2)))
