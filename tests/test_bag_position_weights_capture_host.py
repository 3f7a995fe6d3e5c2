"""Position weights in the captured bag-mode step: what can be checked without a GPU -- the new C-ABI entries and their struct,
their argument checks (every one returns before the context is touched or anything is launched), ops.BagSide's two sources, the
refusal function's opt-in, and the train driver's new flag at argument parsing."""
import ctypes
import re
import subprocess
import sys

import pytest
import torch

from conftest import GOLD, ROOT

import jodalrob_twotower_amd as tt
from jodalrob_twotower_amd import _lib, ops
from jodalrob_twotower_amd.cat_embed import CategoricalEmbedder, refuse_learned_weights

META = str(GOLD / "synthetic_metadata.csv")
ENTRIES = ("tt_embed_bag_fwd_posw", "tt_embed_bag_fwd_cap_posw")
TT_ERR_INVALID_ARG, TT_ERR_UNSUPPORTED = -1, -4                 # include/twotower.h


def test_symbols_in_header_and_library():
    header = (ROOT / "include" / "twotower.h").read_text()
    lib = _lib.load()
    for name in ENTRIES:
        assert re.search(rf"^\s*int\s+{name}\s*\(", header, flags=re.M), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert re.search(r"#define TT_ABI_VERSION 2\b", header)                        # entries were added, none changed
    assert _lib.SIGNATURES["tt_embed_bag_fwd_posw"] == _lib.SIGNATURES["tt_embed_bag_fwd_cap_posw"]
    # the _w entries' arguments with the weight pointers' array replaced by the sources' array
    w, pw = _lib.SIGNATURES["tt_embed_bag_fwd_w"][1], _lib.SIGNATURES["tt_embed_bag_fwd_posw"][1]
    assert len(w) == len(pw) and [i for i, (x, y) in enumerate(zip(w, pw)) if x is not y] == [9]
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct tt_bag_weight_src \{(.*?)\} tt_bag_weight_src;", header, flags=re.S).group(1),
                  flags=re.S)
    assert re.findall(r"(\w+);", body) == [f[0] for f in _lib.BagWeightSrc._fields_]
    assert ctypes.sizeof(_lib.BagWeightSrc) == 4 * 8 + 8
    # the index and its clamp have one definition, shared by the expansion launch and the lookup
    csrc = ROOT / "jodalrob-twotower_amd" / "csrc"
    assert "pw_index_at" in (csrc / "tt_bag_pw.h").read_text()
    for f in ("tt_embed_bag.hip", "tt_bag_weight_grad.hip"):
        text = (csrc / f).read_text()
        assert '#include "tt_bag_pw.h"' in text and not re.search(r"int64_t\s+pw_index\w*\s*\(", text), f


class _Args:
    """arguments that pass every check of tt_embed_bag_fwd[_cap]_posw up to the first use of the context: host memory that is never
    read -- each call below must return before that"""

    def __init__(self):
        self.mem = (ctypes.c_char * 8192)()
        base = (ctypes.addressof(self.mem) + 63) // 64 * 64
        self.p = lambda i: _lib.vp(base + 256 * i)
        self.side = (_lib.BagSide * 1)(_lib.BagSide(self.p(1), self.p(2), self.p(3), self.p(4), self.p(5), self.p(6), 24, 5, 3, _lib.TT_F32))
        self.src = _lib.BagWeightSrc(None, self.p(7), self.p(8), self.p(9), 36)

    def call(self, name, src=None, ctx=True, srcs=True, rows=False, w_out=False):
        arr = (_lib.BagWeightSrc * 1)(self.src if src is None else src)
        return getattr(_lib.load(), name)(self.p(0) if ctx else None, self.p(10), 100, 8, self.side, 1, 4,
                                          self.p(11) if rows else None, self.p(12) if rows else None, arr if srcs else None,
                                          self.p(13) if w_out else None, None)


@pytest.mark.parametrize("name", ENTRIES)
def test_c_entries_check_their_arguments_before_any_launch(name):
    lib, a = _lib.load(), _Args()
    n0 = lib.tt_launch_count()
    S = _lib.BagWeightSrc
    cases = [
        (dict(ctx=False), TT_ERR_INVALID_ARG, "NULL argument"),
        (dict(srcs=False), TT_ERR_INVALID_ARG, "NULL weight sources"),
        (dict(src=S(a.p(14), a.p(7), a.p(8), a.p(9), 36)), TT_ERR_INVALID_ARG, "both per-id weights and a position-weight parameter"),
        (dict(src=S(None, a.p(7), None, a.p(9), 36)), TT_ERR_INVALID_ARG, "without pw_offset / pw_len"),
        (dict(src=S(None, a.p(7), a.p(8), None, 36)), TT_ERR_INVALID_ARG, "without pw_offset / pw_len"),
        (dict(src=S(None, a.p(7), a.p(8), a.p(9), 0)), TT_ERR_INVALID_ARG, "bad n_param"),
        (dict(src=S(None, a.p(7), a.p(8), a.p(9), 1 << 31)), TT_ERR_INVALID_ARG, "bad n_param"),
        (dict(src=S(None, _lib.vp(a.p(7).value + 2), a.p(8), a.p(9), 36)), TT_ERR_UNSUPPORTED, "4-byte aligned"),
        (dict(rows=True), TT_ERR_INVALID_ARG, "tt_embed_bag_fwd_posw: rows_out with weights on side 0 needs w_out"),
    ]
    for kw, rc, what in cases:
        assert a.call(name, **kw) == rc, (kw, what)
        assert what in lib.tt_last_error_string().decode(), (what, lib.tt_last_error_string())
    assert lib.tt_launch_count() == n0


def test_bag_side_takes_one_source():
    dev = torch.device("cpu")
    K, B, E = 3, 2, 8
    i64, i32 = (lambda *v: torch.tensor(v, dtype=torch.int64)), (lambda *v: torch.tensor(v, dtype=torch.int32))
    pw = ops.BagPosWeights(torch.ones(6), i32(0, 4, -1), i32(4, 2, 0))
    mk = lambda **kw: ops.BagSide(torch.zeros(6, dtype=torch.int64), torch.ones(B * K, dtype=torch.int64), i64(0, 5, 9), i64(5, 4, 3),
                                  i32(1, 0, 0), torch.zeros(B, K * E), K, **kw)
    assert mk().pos_weights is None and mk().weights is None
    ops._check_bag_side(0, mk(pos_weights=pw), B, E, dev)
    ops._check_bag_side(0, mk(weights=torch.ones(6)), B, E, dev)
    with pytest.raises(ValueError, match="side 1: per-id weights and a position-weight source on one side"):
        ops._check_bag_side(1, mk(weights=torch.ones(6), pos_weights=pw), B, E, dev)
    for bad, what in ((ops.BagPosWeights(torch.ones(6, dtype=torch.float64), pw.pw_offset, pw.pw_len), "float32 vector"),
                      (ops.BagPosWeights(torch.ones(2, 3), pw.pw_offset, pw.pw_len), "float32 vector"),
                      (ops.BagPosWeights(torch.ones(0), pw.pw_offset, pw.pw_len), "non-empty"),
                      (ops.BagPosWeights(torch.ones(12)[::2], pw.pw_offset, pw.pw_len), "contiguous"),
                      (ops.BagPosWeights(pw.param, i32(0, 4), pw.pw_len), "pw_offset must be a contiguous int32 tensor of 3"),
                      (ops.BagPosWeights(pw.param, pw.pw_offset, i64(4, 2, 0)), "pw_len must be a contiguous int32 tensor of 3")):
        with pytest.raises(ValueError, match=what):
            ops._check_bag_side(0, mk(pos_weights=bad), B, E, dev)
    assert ops.BagPlan._fields[-1] == "offsets" and ops.BagPlan._field_defaults["offsets"] is None


def test_static_kjt_gets_the_source_and_the_refusal_has_an_opt_in(schema_syn):
    import inspect
    from jodalrob_twotower_amd.graph import GraphedTrainStep
    kn, kc = schema_syn["notice"]["categorical"], schema_syn["company"]["categorical"]
    emb = CategoricalEmbedder(kc, META, "company", embedding_dim=4, device="cpu", pooling="sum").add_position_weights({kc[0]: 3})
    n = 2 * len(kc)
    kjt = tt.build_bag_kjt(kc, values=torch.zeros(n, dtype=torch.long), lengths=torch.ones(n, dtype=torch.long))
    kjt.bag_count = torch.tensor([n], dtype=torch.int32)            # what a captured step attaches to its static KJT
    src = emb.bag_weights(kjt)
    assert isinstance(src, ops.BagPosWeights) and src.param is emb.position_weight
    assert src.pw_offset is emb._pw_offset and src.pw_len is emb._pw_len
    with pytest.raises(ValueError, match="run through the towers"):
        emb(kjt)
    wk = tt.build_bag_kjt(kc, values=torch.zeros(n, dtype=torch.long), lengths=torch.ones(n, dtype=torch.long), weights=torch.ones(n))
    wk.bag_count = kjt.bag_count
    with pytest.raises(ValueError, match="one source of weights per embedder"):
        emb.bag_weights(wk)
    assert inspect.signature(GraphedTrainStep.__init__).parameters["learned_weights"].default is False
    mk = lambda **kw: tt.create_two_tower_train_task(kn, kc, metadata_path=META, categorical_embedding_dim=4, notice_dense_input_dim=3,
                                                     company_dense_input_dim=2, tower_hidden_dims=[8, 4], final_embedding_dim=4,
                                                     device="cpu", **kw)
    task, plain = mk(categorical_pooling="sum", categorical_position_weights={kc[0]: 2}), mk(categorical_pooling="sum")
    refuse_learned_weights(task, "GraphedTrainStep", learned=True)
    with pytest.raises(ValueError, match=r"GraphedTrainStep\(learned_weights=True\): no embedder of the model learns position weights"):
        refuse_learned_weights(plain, "GraphedTrainStep", learned=True)
    with pytest.raises(ValueError, match="GraphedTrainStep does not support learned position weights.*eager step"):
        refuse_learned_weights(task, "GraphedTrainStep")
    w = torch.ones(n, requires_grad=True)
    gk = tt.build_bag_kjt(kc, values=torch.zeros(n, dtype=torch.long), lengths=torch.ones(n, dtype=torch.long), weights=w)
    with pytest.raises(ValueError, match="weights that require grad.*eager step"):
        refuse_learned_weights(task, "GraphedTrainStep", [gk], learned=True)


def test_train_driver_takes_the_new_flag_at_argument_parsing():
    run = lambda *args: subprocess.run([sys.executable, str(ROOT / "scripts" / "train.py"), *args], capture_output=True, text=True, timeout=300)
    pool = ["--pool", "rgncd=mean", "--pool-position-weights", "4"]
    # accepted: parsing passes the position-weight checks and stops at a later one (no training is started)
    for extra in (["--pool-capture", "2"], ["--pool-store", "--fast"]):
        r = run(*pool, *extra, "--pool-position-weights-captured", "--log-interval", "0")
        assert r.returncode == 2 and "--log-interval must be >= 1" in r.stderr and "--pool-position-weights:" not in r.stderr, r.stderr[-400:]
    r = run("--pool", "rgncd=mean", "--pool-capture", "2", "--pool-position-weights-captured")
    assert r.returncode == 2 and "--pool-position-weights-captured needs --pool-position-weights" in r.stderr
    r = run(*pool, "--pool-position-weights-captured")
    assert r.returncode == 2 and "--pool-position-weights-captured needs a captured step" in r.stderr
    r = run(*pool, "--pool-capture", "2", "--pool-position-weights-captured", "--pool-weights")
    assert r.returncode == 2 and "one source of weights per embedder" in r.stderr
