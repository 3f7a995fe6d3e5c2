#!/usr/bin/env python3
"""Training driver on the MI355X path -- the counterpart of the reference's scripts/train.py
(config dict :84-134, Adam + LambdaLR warm-up :231-242, loop :313-352, validation :367-423, evaluator
:444-452, checkpoints :497-551, results CSV :24-75).  The reference driver needs PostgreSQL
(DatabaseConnector(), :159); this one takes the same config keys and a synthetic feature/pair source.

    python scripts/train.py [--resume PATH] [--steps N] [--batch-size B] [--fast]

--fast: the loop the MI355X path is built for -- bf16 towers and score operands, row-sparse table gradients, FusedAdam, the
whole step replayed from ONE captured HIP graph, every full batch gathered out of the device-resident feature stores by the
step's own hand-over launch (DevicePairLoader.step_batches -> GraphedTrainStep.step_from_store -> tt_batch_ingest_store): no
batch tensors, nothing per step over PCIe.  Without the flag the loop is the reference's own, statement for statement
(eager forward / backward / optimiser step on the loader's batches, f32 parity kernels).  Either way the run ends like the
reference driver: validation, evaluator report, prediction demo, checkpoints, a results-CSV row; and prints pairs/s over the
whole epoch including evaluation.
"""
from __future__ import annotations

import argparse
import csv
import sys
import tempfile
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "jodalrob-twotower_amd" / "dropin"))

from src.evaluation.evaluator import TwoTowerEvaluator                       # noqa: E402  (same imports as the reference driver)
from src.torchrec_preprocess.schema import build_torchrec_schema_from_meta    # noqa: E402
from src.towers.pairs.unified_bid_data_loader import create_unified_bid_dataloaders  # noqa: E402
from src.towers.two_tower_train_task import create_two_tower_train_task       # noqa: E402
from jodalrob_twotower_amd import synthetic                                   # noqa: E402
from jodalrob_twotower_amd.optim import FusedAdam                             # noqa: E402

# the reference's results CSV, column for column and in its order (scripts/train.py:37-57; pinned by tests/golden/api_surface.json
# "harness" -> "results_csv"): a train_results.csv written here concatenates with one the reference wrote
RESULT_COLUMNS = ["timestamp", "batch_size", "model_params", "embedding_dim", "final_embedding_dim", "hidden_dims", "learning_rate",
                  "epochs", "train_loss", "train_acc", "val_loss", "val_acc", "recall_at_5", "recall_at_10", "mrr", "similarity_gap",
                  "train_batches", "test_batches", "gpu_optimization"]
_FROM_HYPERPARAMS = {"batch_size", "model_params", "embedding_dim", "final_embedding_dim", "hidden_dims", "learning_rate", "epochs",
                     "train_batches", "test_batches", "gpu_optimization"}


def save_training_results(hyperparams, metrics, output_file="train_results.csv"):
    """One row per run appended to `output_file` (reference: scripts/train.py:24-75, same signature and default file).  Missing
    values are written as "N/A" like the reference's `.get(key, "N/A")`.  One deliberate difference: the reference's driver fills
    `final_metrics["recall@5"]` / `["recall@10"]` (:479-480) but its writer reads `recall_at_5` / `recall_at_10` (:50-51), so its
    own two columns are always empty (train_results.csv:2-4); here either spelling is accepted and the columns carry the values."""
    row = {"timestamp": time.strftime("%Y-%m-%d %H:%M:%S")}
    for col in RESULT_COLUMNS[1:]:
        if col in _FROM_HYPERPARAMS:
            v = hyperparams.get(col, "N/A")
            row[col] = str(v) if col == "hidden_dims" else v
        else:
            v = metrics.get(col, metrics.get(col.replace("_at_", "@"), "N/A"))
            row[col] = v
    out = Path(output_file)
    new = not out.exists()
    with open(out, "a", newline="", encoding="utf-8") as f:
        w = csv.DictWriter(f, fieldnames=RESULT_COLUMNS)
        if new:
            w.writeheader()
        w.writerow(row)
    print(f"학습 결과 저장 완료: {out}")
    return row


def save_checkpoint(model, optimizer, epoch, loss, save_dir, is_best=False, is_final=False):
    save_dir = Path(save_dir)
    save_dir.mkdir(parents=True, exist_ok=True)
    ckpt = {"epoch": epoch, "model_state_dict": model.state_dict(), "optimizer_state_dict": optimizer.state_dict(), "loss": loss}
    if not is_final:
        torch.save(ckpt, save_dir / f"checkpoint_epoch_{epoch + 1}.pt")
    if is_best:
        torch.save(ckpt, save_dir / "best_model.pt")
    if is_final:
        torch.save(ckpt, save_dir / "final_model.pt")
        torch.save(model.state_dict(), save_dir / "model_weights.pt")


def load_checkpoint(model, optimizer, checkpoint_path):
    ckpt = torch.load(checkpoint_path, map_location="cuda:0", weights_only=True)
    model.load_state_dict(ckpt["model_state_dict"])
    optimizer.load_state_dict(ckpt["optimizer_state_dict"])
    return ckpt["epoch"] + 1, ckpt["loss"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resume", default=None)
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--entities", type=int, default=10_000)
    ap.add_argument("--pairs", type=int, default=100_000)
    ap.add_argument("--steps", type=int, default=None, help="stop after this many training steps")
    ap.add_argument("--output-dir", default="output/models")
    ap.add_argument("--fast", action="store_true", help="captured step fed from the device stores, bf16 operands, sparse gradients")
    ap.add_argument("--hidden", default="128,64", help="tower_hidden_dims (the reference driver trains 512,256: scripts/train.py:106)")
    ap.add_argument("--final-dim", type=int, default=64)
    ap.add_argument("--epochs", type=int, default=1)
    ap.add_argument("--table-optimizer", choices=["adam", "rowwise_adagrad"], default="adam",
                    help="optimiser of the embedding tables (the towers keep Adam); rowwise_adagrad keeps one float per table row")
    ap.add_argument("--table-lr", type=float, default=None, help="learning rate of the tables under rowwise_adagrad (default: the towers' learning rate)")
    ap.add_argument("--pair-zipf", type=float, default=None,
                    help="synthetic pairs: each pair's company drawn from a Zipf(A) law over company rank (default: uniform)")
    ap.add_argument("--mask-repeats", action="store_true",
                    help="mask the in-batch negatives that repeat a row's notice or company (the repeated-entity mask): the train loader "
                         "attaches each pair's notice / company index (evaluation stays unmasked); combines with --logq-correction")
    ap.add_argument("--mask-known", action="store_true",
                    help="mask every known (notice, company) pair of the TRAIN pair table out of the in-batch softmax: an in-batch company or "
                         "an extra that is a known bidder of a row's notice is no negative of that row (the train loader attaches the cells; "
                         "evaluation stays unmasked); needs --fast (bf16 score kernels); combines with --logq-correction, --extra-negatives and "
                         "--mine-negatives, holds every repeat --mask-repeats would mask and is an error with it or with --pair-weight")
    ap.add_argument("--pair-weight", choices=["inv-notice-count"], default=None,
                    help="per-pair sample weights of the in-batch softmax: inv-notice-count = 1 / (pairs of the row's notice), every notice "
                         "counts once; attached to the train loader only; combines with --mask-repeats and --logq-correction")
    ap.add_argument("--logq-correction", action="store_true",
                    help="logQ sampling-bias correction of the in-batch softmax: log sampling probabilities estimated from the TRAIN pairs, "
                         "attached to the train loader only (evaluation stays uncorrected)")
    ap.add_argument("--extra-negatives", type=int, default=0, metavar="M",
                    help="shared extra negatives: every train batch carries M more company rows, drawn uniformly from the company store, "
                         "that every notice of the batch is contrasted with besides the in-batch companies (mixed negative sampling); "
                         "combines with --mask-repeats and --logq-correction, not with --pair-weight; with --fast the captured step takes "
                         "them through its plain-copy hand-over")
    ap.add_argument("--mine-negatives", type=int, default=0, metavar="E",
                    help="hard-negative mining: before every E-th epoch, mine the train pairs' notices against the whole company catalogue "
                         "with the current weights (score ceiling relative to each notice's own positives, known companies excluded) and "
                         "draw each batch's extras from the rows mined for that batch's notices; needs --extra-negatives M")
    ap.add_argument("--mine-k", type=int, default=64, help="rows searched per notice under the ceiling")
    ap.add_argument("--mine-per-notice", type=int, default=8, help="rows kept per notice (the best of the --mine-k)")
    ap.add_argument("--mine-ceiling", type=float, nargs=2, default=(0.95, 0.0), metavar=("A", "B"),
                    help="score ceiling A * s_min + B, s_min the lowest score of the notice's known companies")
    ap.add_argument("--hard-fraction", type=float, default=1.0, metavar="F", help="share of the M extras drawn from the mined rows")
    ap.add_argument("--results-csv", default="train_results.csv", help="the results CSV (reference: train_results.csv in the working directory)")
    ap.add_argument("--pool", nargs="+", default=None, metavar="KEY=MODE",
                    help="multi-valued categorical features: the named keys (either tower) hold ragged bags of ids pooled by MODE = sum | "
                         "mean (bag mode; eager loop only).  The synthetic stores hold one id per key: every training batch draws "
                         "--pool-length more ids per bag on average; evaluation feeds each entity's own id as a bag of one")
    ap.add_argument("--pool-length", type=float, default=4.0, help="mean bag length of the --pool keys' synthetic bags")
    ap.add_argument("--pool-weights", action="store_true",
                    help="with --pool: every id of the pooled towers' bags carries a weight (the KJT's weights(): U[0.5, 1.5), a bag's first "
                         "id weighing 1) -- the weighted pooled lookup, in the eager loop and with --pool-capture; not with --pool-store "
                         "(the bag stores hold ids alone)")
    ap.add_argument("--pool-capture", nargs="?", type=float, const=2.0, default=None, metavar="FACTOR",
                    help="with --pool: the pooled loop runs as a captured step (GraphedTrainStep(bag_capacity=...)) whose static id "
                         "buffers hold FACTOR (default 2) times the first batch's ids per bag-mode side; a batch that does not fit "
                         "takes the eager step and is counted")
    ap.add_argument("--pool-store", action="store_true",
                    help="with --pool: every entity's bags are drawn ONCE (the --pool keys: Poisson(--pool-length) ids, the entity's own "
                         "first) into device-resident bag stores (DeviceBagFeatureStore) that training AND evaluation read, so the "
                         "model is evaluated on the bags it is trained on.  The model is built as under --fast (bf16 operands, sparse "
                         "gradients) with or without it; with --fast the epoch runs through step_batches on a step captured with "
                         "--pool-capture FACTOR (default 2) times the pair table's mean ids per batch, fed by the stores' own hand-over")
    ap.add_argument("--seed", type=int, default=None, help="seed torch's generators (weights, dropout) before the model is built")
    ap.add_argument("--dropout-rate", type=float, default=0.1, help="the towers' dropout rate (reference: 0.1)")
    ap.add_argument("--log-interval", type=int, default=20, help="steps between the loop's progress lines (reference: 20)")
    ap.add_argument("--pool-store-weights", action="store_true",
                    help="with --pool ... --pool-store: the bag stores also keep one weight per id (U[0.5, 1.5), a bag's first id "
                         "weighing 1), drawn once with the bags -- training (also --fast: the store-fed hand-over moves the weights "
                         "with the ids) and evaluation read them")
    ap.add_argument("--pool-position-weights", type=int, default=None, metavar="MAXLEN",
                    help="with --pool: every pooled key learns one weight per bag position (MAXLEN of them, initialised to 1; later "
                         "positions share the last) -- the eager loop only: not with --pool-weights / --pool-store-weights (one source "
                         "of weights per embedder), --pool-capture or --pool-store --fast (unless --pool-position-weights-captured)")
    ap.add_argument("--pool-position-weights-captured", action="store_true",
                    help="with --pool-position-weights and --pool-capture or --pool-store --fast: the captured step trains the position "
                         "weights itself (GraphedTrainStep(learned_weights=True)): the pooled lookup reads them by position, their "
                         "gradient is formed over the capacity inside the graph")
    a = ap.parse_args()
    pooling = None
    if a.pool_position_weights_captured and a.pool_position_weights is None:
        ap.error("--pool-position-weights-captured needs --pool-position-weights MAXLEN")
    if a.pool_position_weights_captured and a.pool_capture is None and not (a.pool_store and a.fast):
        ap.error("--pool-position-weights-captured needs a captured step: --pool-capture FACTOR or --pool-store --fast")
    if a.pool_position_weights is not None:
        if not a.pool:
            ap.error("--pool-position-weights needs --pool")
        if a.pool_position_weights < 1:
            ap.error("--pool-position-weights MAXLEN must be >= 1")
        if a.pool_weights or a.pool_store_weights:
            ap.error("--pool-position-weights: not with --pool-weights / --pool-store-weights -- one source of weights per embedder")
        if a.pool_capture is not None and not a.pool_position_weights_captured:
            ap.error("--pool-position-weights: not with --pool-capture -- the captured step forms no gradient for weights; use the eager loop")
        if a.pool_store and a.fast and not a.pool_position_weights_captured:
            ap.error("--pool-position-weights: not with --pool-store --fast -- the captured step forms no gradient for weights; use the eager loop")
    if a.pool_store and not a.pool:
        ap.error("--pool-store needs --pool")
    if a.pool_weights and not a.pool:
        ap.error("--pool-weights needs --pool")
    if a.pool_weights and a.pool_store:
        ap.error("--pool-weights: not with --pool-store -- the device-resident bag stores hold ids alone (weighted stores are not built yet)"
                 "; --pool-store-weights draws per-entity weights into the stores")
    if a.pool_store_weights and not a.pool_store:
        ap.error("--pool-store-weights needs --pool ... --pool-store")
    if a.pool_store and a.fast and (a.extra_negatives or a.mask_known):
        ap.error("--pool-store --fast: no store-fed hand-over with --extra-negatives or --mask-known")
    if a.pool:
        if a.fast and not a.pool_store:
            ap.error("--pool needs the eager loop: a captured step's static id buffers hold exactly B*K ids (not with --fast)")
        pooling = {}
        for item in a.pool:
            key, _, mode = item.partition("=")
            if mode not in ("sum", "mean"):
                ap.error(f"--pool {item!r}: expected KEY=sum or KEY=mean")
            pooling[key] = mode
    if a.pool_capture is not None and not a.pool:
        ap.error("--pool-capture needs --pool")
    if a.pool_capture is not None and a.pool_capture < 1.0:
        ap.error("--pool-capture FACTOR must be >= 1")
    if a.log_interval < 1:
        ap.error("--log-interval must be >= 1")
    if a.mask_known and (a.mask_repeats or a.pair_weight):
        ap.error("--mask-known does not combine with --mask-repeats (its cells hold every repeat) or --pair-weight")
    if a.mask_known and not a.fast:
        ap.error("--mask-known needs --fast: masked cells run on the bf16 score kernels only (the f32 parity path has no cells form)")
    if a.mine_negatives < 0:
        ap.error("--mine-negatives must be >= 0")
    if not a.extra_negatives and (a.mine_negatives or a.hard_fraction != 1.0):
        ap.error("--mine-negatives / --hard-fraction need --extra-negatives M")
    config = {"batch_size": a.batch_size, "test_split": 0.2, "shuffle_seed": 42, "pair_limit": a.pairs,
              "categorical_embedding_dim": 32, "notice_dense_input_dim": 256, "company_dense_input_dim": 128,
              "tower_hidden_dims": [int(h) for h in a.hidden.split(",")], "final_embedding_dim": a.final_dim, "dropout_rate": a.dropout_rate,
              "temperature": 1.0, "loss_type": "cross_entropy", "learning_rate": 1e-3, "weight_decay": 1e-5, "num_epochs": a.epochs,
              "warmup_ratio": 0.05, "log_interval": a.log_interval, "output_dir": a.output_dir,
              "gpu_optimization": ("MI355X HIP graph replay + device-resident stores + bf16 MFMA / sparse FusedAdam" if a.fast
                                   else "MI355X HIP kernels, eager, f32 parity mode")}
    device = torch.device("cuda:0")
    if a.seed is not None:
        torch.manual_seed(a.seed)
    real = synthetic.load_real_schema(ROOT / "jodalrob-twotower_amd" / "schema_real.json")
    tmp = Path(tempfile.mkdtemp(prefix="tt_train_"))
    meta_rows = [synthetic.META_HEADER]
    for side in ("notice", "company"):
        for c in real[side]["pk_cols"]:
            meta_rows.append(f"{side},{c},text,Y,,,,0,,Y,Y,,")
        for c in real[side]["numeric"]:
            meta_rows.append(f"{side},{c},numeric,Y,,,,0,,,,,")
        for c, v in zip(real[side]["categorical"], real[side]["vocab_sizes"]):
            meta_rows.append(f"{side},{c},text,Y,,Y,{v - 10},0,,,,,")
        for c in real[side]["text"]:
            meta_rows.append(f"{side},{c},text,Y,,N,,0,,,,,")
    meta = tmp / "metadata.csv"
    meta.write_text("\n".join(meta_rows) + "\n", encoding="utf-8")
    schema = build_torchrec_schema_from_meta(notice_table="notice", company_table="company", pair_table="bid_two_tower",
                                             pair_notice_id_cols=["bidntceno", "bidntceord"], pair_company_id_cols=["bizno"],
                                             metadata_path=str(meta))
    source = synthetic.SyntheticSource(a.entities, a.entities, a.pairs, real["notice"]["vocab_sizes"], real["company"]["vocab_sizes"],
                                       pair_zipf_alpha=a.pair_zipf)
    train_loader, test_loader = create_unified_bid_dataloaders(source, schema, batch_size=config["batch_size"],
                                                               test_split=config["test_split"], shuffle_seed=config["shuffle_seed"],
                                                               test_mode=True, pair_limit=config["pair_limit"], device=device)
    if a.pool_store:                                     # the towers that pool read per-entity bags, drawn once; both loaders share them
        bag_stores = [synthetic.bag_store(st, real[side]["vocab_sizes"], pooling, a.pool_length, seed=config["shuffle_seed"] + i,
                                          weights="uniform" if a.pool_store_weights else None)
                      if any(k in pooling for k in st.keys) else st
                      for i, (side, st) in enumerate((("notice", train_loader.notice), ("company", train_loader.company)))]
        for ld in (train_loader, test_loader):
            ld.notice, ld.company = bag_stores
    if a.mask_repeats:
        train_loader.set_mask_repeats(True)
    if a.pair_weight == "inv-notice-count":
        from jodalrob_twotower_amd.pair_weights import inverse_count_weights
        train_loader.set_pair_weight(inverse_count_weights(train_loader.pairs, "notice"))
    if a.logq_correction:                                # exact: batches are uniform draws from this fixed pair list
        from jodalrob_twotower_amd.sampling_bias import log_sampling_probs
        tp = train_loader.pairs
        train_loader.set_log_q((log_sampling_probs(tp[:, 0], len(train_loader.notice)),
                                log_sampling_probs(tp[:, 1], len(train_loader.company))))
    if a.extra_negatives:
        train_loader.set_extra_negatives(a.extra_negatives)
    if a.mask_known:
        train_loader.set_mask_known(True)
    train_task = create_two_tower_train_task(schema.notice.categorical, schema.company.categorical, metadata_path=str(meta),
                                             categorical_embedding_dim=config["categorical_embedding_dim"],
                                             notice_dense_input_dim=config["notice_dense_input_dim"],
                                             company_dense_input_dim=config["company_dense_input_dim"],
                                             tower_hidden_dims=config["tower_hidden_dims"],
                                             final_embedding_dim=config["final_embedding_dim"], dropout_rate=config["dropout_rate"],
                                             temperature=config["temperature"], loss_type=config["loss_type"], device=device,
                                             categorical_pooling=pooling,
                                             categorical_position_weights=({k: a.pool_position_weights for k in pooling}
                                                                           if a.pool_position_weights is not None else None),
                                             **(dict(embedding_grad="sparse", score_dtype="bf16", mlp_dtype="bf16") if (a.fast or a.pool_store) else {}))
    optimizer = FusedAdam.for_task(train_task, lr=config["learning_rate"], weight_decay=config["weight_decay"],
                                   table_optimizer=a.table_optimizer, table_lr=a.table_lr)
    warmup_steps = max(1, int(len(train_loader) * config["warmup_ratio"]))
    scheduler = torch.optim.lr_scheduler.LambdaLR(optimizer, lambda s: s / warmup_steps if s < warmup_steps else 1.0, last_epoch=-1)
    start_epoch = 0
    if a.resume:
        start_epoch, _ = load_checkpoint(train_task, optimizer, a.resume)
    total_params = sum(p.numel() for p in train_task.parameters())
    print(f"params: {total_params:,}  train batches: {len(train_loader)}  warm-up steps: {warmup_steps}")
    evaluator = TwoTowerEvaluator(device=device)
    t0, steps, best_val_loss = time.time(), 0, float("inf")
    if start_epoch >= config["num_epochs"]:
        config["num_epochs"] = start_epoch + 1           # resumed after the last epoch: run one more

    pool_step, pool_eager = None, 0                      # --pool-capture: the captured bag-mode step; batches that took the eager one

    def eager_step(batch):
        nonlocal pool_step, pool_eager
        if graphed is not None and pooling:              # --pool-store --fast: a batch step_batches could not replay
            pool_eager += 1
        if pooling and not a.pool_store:                 # ragged bags for the pooled keys, drawn per step (seeded by the step number)
            batch = dict(batch)
            for side in ("notice", "company"):
                weighted = a.pool_weights and any(k in pooling for k in batch[side]["kjt"].keys())      # (a tower that pools nothing takes none)
                batch[side] = dict(batch[side], kjt=synthetic.ragged_bags(batch[side]["kjt"], real[side]["vocab_sizes"], pooling,
                                                                          a.pool_length, seed=config["shuffle_seed"] + steps,
                                                                          weights="uniform" if weighted else None))
        if a.pool_capture is not None and train_task.training and graphed is None:
            if pool_step is None:                        # captured on the first batch (its warm-up leaves no trace: preserve_state)
                import math
                from jodalrob_twotower_amd.graph import GraphedTrainStep
                model = train_task.two_tower_model
                caps = {side: max(1, math.ceil(a.pool_capture * batch[side]["kjt"].values().numel()))
                        for side, tw in (("notice", model.notice_tower), ("company", model.company_tower)) if tw.categorical_embedder.bag_mode}
                pool_step = GraphedTrainStep(train_task, optimizer, batch, warmup=1, bag_capacity=caps,
                                             learned_weights=a.pool_position_weights_captured)
                print(f"--pool-capture: captured with bag_capacity = {caps}")
            fits = batch["notice"]["dense"].shape == pool_step.static["notice"]["dense"].shape and \
                all(batch[side]["kjt"].values().numel() <= cap for side, cap in pool_step.bag_capacity.items())
            if fits:
                return pool_step.step(batch)
            pool_eager += 1                              # a fuller (or the epoch's last, smaller) batch
        optimizer.zero_grad()
        result = train_task(batch, return_metrics=True)
        result["loss"].backward()
        optimizer.step()
        return result

    graphed, ragged = None, None
    if a.fast and len(train_loader) > 1:                 # (a loader of one ragged batch has nothing to capture)
        from jodalrob_twotower_amd.graph import GraphedTrainStep
        train_task.train()
        state, neg_state = train_loader._gen.get_state(), train_loader._neg_gen.get_state()
        example = next(iter(train_loader))               # shapes only: the capture's warm-up steps leave no trace (preserve_state)
        train_loader._gen.set_state(state)
        train_loader._neg_gen.set_state(neg_state)
        # masked cells: room for twice the example epoch's fullest batch (a fuller one goes through the eager step: step_batches)
        cap = {"cell_capacity": max(1024, 2 * train_loader.max_cells)} if a.mask_known else {}
        if a.pool_store:                                 # bag_capacity: FACTOR times the pair table's mean ids per batch (the example fits)
            import math
            factor = 2.0 if a.pool_capture is None else a.pool_capture
            caps = {side: max(math.ceil(factor * float(st.run_lengths[train_loader.pairs[:, col]].sum()) * config["batch_size"] / len(train_loader.pairs)),
                              example[side]["kjt"].values().numel(), 1) for side, st, col in train_loader.bag_stores()}
            cap["bag_capacity"] = caps
            if a.pool_position_weights_captured:
                cap["learned_weights"] = True
            print(f"--pool-store: captured with bag_capacity = {caps}")
        graphed = GraphedTrainStep(train_task, optimizer, example, warmup=1, accumulate_metrics=True, **cap)
        rag = train_loader.ragged_example()              # the epoch's last, smaller batch gets a captured step of its own size:
        if rag is not None and rag["notice"]["dense"].shape[0] >= 2:       # launched eagerly it costs six full steps of host time
            ragged = GraphedTrainStep(train_task, optimizer, rag, warmup=1, accumulate_metrics=True, **cap)
    if a.fast:                                           # one-off: capture the evaluation pass too (outside the epoch clock, like the step's capture)
        evaluator._fast_eval(train_task, test_loader)
    log = _AsyncLog(device) if a.fast else None
    torch.cuda.synchronize()
    pairs_seen, t_loop, t_train, t_eval = 0, time.time(), 0.0, 0.0
    avg_train_loss = avg_train_acc = avg_val_loss = avg_val_acc = float("nan")
    val = {}
    stop = False
    for epoch in range(start_epoch, config["num_epochs"]):
        print(f"\nEpoch {epoch + 1}/{config['num_epochs']}")
        t_e0 = time.time()
        if a.mine_negatives and (epoch - start_epoch) % a.mine_negatives == 0:
            from jodalrob_twotower_amd.hard_negatives import mine_hard_negatives
            mined = mine_hard_negatives(train_task, train_loader.notice, train_loader.company, train_loader.pairs, k=a.mine_k,
                                        per_notice=a.mine_per_notice, ceiling=tuple(a.mine_ceiling), seed=config["shuffle_seed"] + epoch)
            train_loader.set_extra_negatives(a.extra_negatives, mined=mined, hard_fraction=a.hard_fraction)
            torch.cuda.synchronize()
            n_mined = int((mined.table >= 0).sum())
            print(f"mined {n_mined} hard negatives for {int((mined.table[:, 0] >= 0).sum())} notices in {time.time() - t_e0:.2f} s")
        train_task.train()
        train_losses, train_accuracies, n_epoch_steps = [], [], 0
        for g in (graphed, ragged):
            if g is not None:
                g.metric_sums.zero_()
        results = train_loader.step_batches(graphed, eager_step, ragged) if graphed is not None else (eager_step(b) for b in train_loader)
        for result in results:
            scheduler.step()
            steps += 1
            n_epoch_steps += 1
            pairs_seen += config["batch_size"]
            if graphed is None:                          # the reference's loop reads loss and accuracy every step (:335-336)
                train_losses.append(result["loss"].item())
                train_accuracies.append(result["accuracy"].item())
                if steps % config["log_interval"] == 0:
                    pos, neg = result["positive_similarity_mean"].item(), result["negative_similarity_mean"].item()
                    gap = result["similarity_gap"].item()
                    print(f"step {steps:5d}  loss {train_losses[-1]:.4f}  acc {train_accuracies[-1]:.4f}  pos {pos:.3f}  neg {neg:.3f}  "
                          f"z-gap {gap / max(abs(neg) + 1e-8, 1e-8):.2f}")
            elif steps % config["log_interval"] == 0:    # fast loop: the figures travel to the host behind the step, nobody waits
                log.post(steps, result.out8)
                log.drain()
            if a.steps and steps >= a.steps:
                stop = True
                break
        if graphed is not None:                          # epoch means from the in-replay sums: ONE host sync per epoch
            sums = graphed.metric_sums.clone()
            if ragged is not None:
                sums += ragged.metric_sums
            sums = sums.cpu()
            log.drain(wait=True)
            # (a ragged batch that went through eager_step is not in the sums: with `ragged` captured there is none)
            avg_train_loss, avg_train_acc = float(sums[0]) / max(n_epoch_steps, 1), float(sums[1]) / max(n_epoch_steps, 1)
        else:
            avg_train_loss = sum(train_losses) / max(len(train_losses), 1)                  # :357-358
            avg_train_acc = sum(train_accuracies) / max(len(train_accuracies), 1)
        torch.cuda.synchronize()
        t_e1 = time.time()
        # the library's sticky device error word (a chained plan launch that gave up, a fused row outside its table): read where the host
        # has synchronised anyway; a raised word invalidates the epoch's steps (include/twotower.h: tt_ctx_check_device_errors)
        from jodalrob_twotower_amd import _lib as _tt_lib
        _tt_lib.check_device_errors(torch.device(device))
        print(f"Train - Loss: {avg_train_loss:.4f}, Accuracy: {avg_train_acc:.3f}")
        # validation (:362-423): mean loss / accuracy over the test loader's batches, model in eval mode
        avg_val_loss = avg_train_loss
        if len(test_loader) > 0:
            if a.fast:                                   # the captured evaluation pass gives the same two means (and the ranks on top)
                val = evaluator.evaluate_comprehensive(train_task, test_loader, verbose=False)
                avg_val_loss, avg_val_acc = val["loss"], val["accuracy"]
            else:
                train_task.eval()
                vl, va = [], []
                with torch.no_grad():
                    for batch in test_loader:
                        result = train_task(batch, return_metrics=True)
                        vl.append(result["loss"].item())
                        va.append(result["accuracy"].item())
                avg_val_loss, avg_val_acc = sum(vl) / len(vl), sum(va) / len(va)
            print(f"Val   - Loss: {avg_val_loss:.4f}, Accuracy: {avg_val_acc:.3f}")
        torch.cuda.synchronize()
        t_train, t_eval = t_train + (t_e1 - t_e0), t_eval + (time.time() - t_e1)
        save_checkpoint(train_task, optimizer, epoch, avg_val_loss, config["output_dir"])                    # :426
        if avg_val_loss < best_val_loss:                                                                      # :429-432
            best_val_loss = avg_val_loss
            save_checkpoint(train_task, optimizer, epoch, avg_val_loss, config["output_dir"], is_best=True)
            print(f"새로운 최고 성능! Loss: {avg_val_loss:.4f}")
        if stop:
            break
    torch.cuda.synchronize()
    t_epochs = time.time() - t_loop
    if a.pool_store and graphed is not None:
        print(f"--pool-store: {steps - pool_eager} captured steps, {pool_eager} batches took the eager step "
              f"({train_loader.eager_bag_batches} over the capacity)")
    elif a.pool_capture is not None:
        print(f"--pool-capture: {steps - pool_eager} captured steps, {pool_eager} batches took the eager step")
        if pool_step is not None:
            pool_step.close()
    print(f"throughput: {pairs_seen / t_epochs:,.0f} pairs/s over {steps} steps incl. evaluation "
          f"({'fast: captured step fed from the device stores' if a.fast else 'eager reference loop'}); "
          f"training {t_train * 1e3:.1f} ms = {pairs_seen / max(t_train, 1e-9):,.0f} pairs/s = {t_train * 1e3 / max(steps, 1):.4f} ms/step, "
          f"evaluation {t_eval * 1e3:.1f} ms ({len(test_loader)} batches), checkpoints {max(t_epochs - t_train - t_eval, 0.0) * 1e3:.1f} ms")
    # final evaluation + prediction demo (:441-452)
    print("\n=== 최종 평가 및 추론 테스트 ===")
    if len(test_loader) > 0:
        print("테스트 데이터 종합 평가:")
        test_metrics = evaluator.evaluate_comprehensive(train_task, test_loader, verbose=True)
    else:
        print("훈련 데이터 샘플로 평가:")
        test_metrics = evaluator.evaluate_single_batch(train_task, next(iter(train_loader)), verbose=True)
    evaluator.demonstrate_predictions(train_task, next(iter(train_loader)), top_k=10)
    for g in (graphed, ragged):
        if g is not None:
            g.close()
    evaluator.close()                                    # (captured evaluation graphs)
    torch.cuda.synchronize()
    # results CSV (:455-487): the reference's two dicts, its columns
    print("\n=== 학습 결과 기록 ===")
    hyperparams = {"batch_size": config["batch_size"], "model_params": total_params, "embedding_dim": config["categorical_embedding_dim"],
                   "final_embedding_dim": config["final_embedding_dim"], "hidden_dims": config["tower_hidden_dims"],
                   "learning_rate": config["learning_rate"], "weight_decay": config["weight_decay"], "dropout_rate": config["dropout_rate"],
                   "temperature": config["temperature"], "epochs": config["num_epochs"], "train_batches": len(train_loader),
                   "test_batches": len(test_loader), "gpu_optimization": config["gpu_optimization"]}
    has_test = len(test_loader) > 0
    final_metrics = {"train_loss": avg_train_loss, "train_acc": avg_train_acc,
                     "val_loss": avg_val_loss if has_test else "N/A", "val_acc": avg_val_acc if has_test else "N/A",
                     "recall@5": test_metrics.get("recall@5", "N/A") if has_test else "N/A",
                     "recall@10": test_metrics.get("recall@10", "N/A") if has_test else "N/A",
                     "mrr": test_metrics.get("mrr", "N/A") if has_test else "N/A",
                     "similarity_gap": test_metrics.get("similarity_gap", "N/A") if has_test else "N/A"}
    save_training_results(hyperparams, final_metrics, a.results_csv)
    save_checkpoint(train_task, optimizer, config["num_epochs"] - 1, 0.0, config["output_dir"], is_final=True)      # :490-491
    print(f"done: {steps} steps in {time.time() - t0:.1f}s; results appended to {a.results_csv}")


class _AsyncLog:
    """Progress lines of the fast loop without stalling it: the step's eight figures (out8) are copied into a pinned host slot on
    the step's stream, an event marks the copy, and a line is printed once its event has passed -- a step or two later."""

    def __init__(self, device, slots: int = 8):
        self.host = torch.zeros(slots, 8, dtype=torch.float32).pin_memory()
        self.pending, self.slots, self.n = [], slots, 0

    def post(self, step, out8):
        if len(self.pending) >= self.slots:
            self.drain(wait=True)
        i = self.n % self.slots
        self.n += 1
        self.host[i].copy_(out8, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.pending.append((step, i, ev))

    def drain(self, wait: bool = False):
        while self.pending and (wait or self.pending[0][2].query()):
            step, i, ev = self.pending.pop(0)
            ev.synchronize()
            loss, acc, pos, neg, gap = (float(x) for x in self.host[i, :5])
            print(f"step {step:5d}  loss {loss:.4f}  acc {acc:.4f}  pos {pos:.3f}  neg {neg:.3f}  z-gap {gap / max(abs(neg) + 1e-8, 1e-8):.2f}")


if __name__ == "__main__":
    main()
