"""Host-side tests of score_dtype = "bf16x3" (split-bf16 score operands): the value is accepted wherever score_dtype is
(TT_SCORE_DTYPE, the task, CatalogIndex -- which maps it to its exact fp32 sweep), unknown strings are still refused, the
packing size is twice the bf16 one, and the new C entries are declared and exported."""
import pytest
import torch

from conftest import ROOT
from jodalrob_twotower_amd import _lib

X3_SYMBOLS = ("tt_score_pack_x3_bytes", "tt_score_pack2_bf16x3", "tt_score_fwd_sym_bf16x3", "tt_score_fwd_bf16x3",
              "tt_score_bwd_bf16x3")


def test_settings_from_env_accepts_bf16x3(monkeypatch):
    from jodalrob_twotower_amd.config import Settings
    monkeypatch.setenv("TT_SCORE_DTYPE", "bf16x3")
    assert Settings.from_env().score_dtype == "bf16x3"


def test_config_docstring_lists_bf16x3():
    from jodalrob_twotower_amd import config
    line = [ln for ln in config.__doc__.splitlines() if "TT_SCORE_DTYPE" in ln and "fp32" in ln][0]
    assert "bf16x3" in line


class _Tower(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.pack_for_score = False
        self.pack_scale = 1.0


class _Model(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.notice_tower, self.company_tower = _Tower(), _Tower()


def test_task_accepts_bf16x3_and_keeps_towers_unpacked():
    from jodalrob_twotower_amd.two_tower_train_task import TwoTowerTrainTask
    m = _Model()
    task = TwoTowerTrainTask(m, temperature=0.07, score_dtype="bf16x3")
    assert task.score_dtype == "bf16x3"
    # the towers' fused tail emits bf16 images only: in this mode the task packs the operands itself
    assert not m.notice_tower.pack_for_score and not m.company_tower.pack_for_score


@pytest.mark.parametrize("bad", ["bf16x2", "x3", "BF16X3", "tf32"])
def test_unknown_score_dtype_is_refused(bad):
    from jodalrob_twotower_amd.two_tower_train_task import TwoTowerTrainTask
    from jodalrob_twotower_amd.retrieval import CatalogIndex
    with pytest.raises(ValueError, match="score_dtype"):
        TwoTowerTrainTask(_Model(), score_dtype=bad)
    with pytest.raises(ValueError, match="score_dtype"):
        CatalogIndex(torch.zeros(4, 8), score_dtype=bad)


def test_catalog_index_maps_bf16x3_to_fp32():
    from jodalrob_twotower_amd.retrieval import CatalogIndex
    C = torch.randn(5, 8)
    idx = CatalogIndex(C, temperature=0.5, score_dtype="bf16x3")       # the fp32 index keeps C itself: no device call
    assert idx.score_dtype == "fp32"
    assert "score_dtype='fp32'" in repr(idx)
    assert torch.equal(idx.data, C)


@pytest.mark.parametrize("R,D", [(0, 1), (1, 1), (63, 3), (65, 64), (4097, 129), (8192, 256)])
def test_pack_x3_bytes_twice_bf16(R, D):
    lib = _lib.load()
    assert lib.tt_score_pack_x3_bytes(R, D) == 2 * lib.tt_score_pack_bytes(R, D)


def test_pack_x3_bytes_rejects_bad_shapes():
    lib = _lib.load()
    for R, D in ((-1, 64), (8, 0), (8, 257)):
        assert lib.tt_score_pack_x3_bytes(R, D) == 0


def test_x3_symbols_declared_and_exported():
    header = (ROOT / "include" / "twotower.h").read_text()
    lib = _lib.load()
    for name in X3_SYMBOLS:
        assert f" {name}(" in header, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
