"""Benchmark driver with the reference's flag names and timing protocol, without DGL.

Mirrors hrt/python/RGNNUtils/RGNNUtils.py (arguments :575-679, training loop :199-433: 5 warm-up steps, forward
and backward(+optimizer.step()) between event pairs, epochs < 3 dropped, of the rest the first quarter dropped,
arithmetic mean, JSON log) and the model stacks of hrt/python/RGAT/models.py:387-512, RGCN/RGCN.py:353-405,
HGT/models.py:246-347.  Datasets: the reference loads DGL/OGB graphs; neither is installable here, so ``-d`` picks a
synthetic graph of the same shape (het_amd/synth.py) or ``--edges_npy`` a ``[3, E]`` (src, dst, etype) array.

    python -m het_amd.train --model rgat -d mag --full_graph_training --num_layers 1 --n_infeat 64 \\
        --num_classes 64 --num_heads 4 --compact_as_of_node_flag --compact_direct_indexing_flag
"""
from __future__ import annotations

import argparse
import contextlib
import json
import sys
import time

import numpy as np
import torch as th
import torch.nn as nn
import torch.nn.functional as F

from .graph import HetGraph
from .layers import HET_EglRelGraphConv_EdgeParallel, HET_HGTLayerHetero, HET_RelGraphEmbed, HET_RGATLayer
from .synth import IntegratedCOO, make_aifb_like, make_mag_like


class HET_RGATModel(nn.Module):
    """hrt/python/RGAT/models.py:387-512: ``num_hidden_layers`` h2h layers + one h2o layer."""

    def __init__(self, num_etypes, h_dim, out_dim, num_heads, num_hidden_layers=1, dropout=0.5, use_self_loop=True,
                 last_layer_act=False, compact_as_of_node_flag=False, compact_direct_indexing_flag=False,
                 multiply_among_weights_first_flag=False, gat_edge_parallel_flag=True, bf16_training=False, keyed_dropout=False):
        super().__init__()
        flags = dict(keyed_dropout=keyed_dropout, compact_as_of_node_flag=compact_as_of_node_flag, compact_direct_indexing_flag=compact_direct_indexing_flag,
                     multiply_among_weights_first_flag=multiply_among_weights_first_flag,
                     gat_edge_parallel_flag=gat_edge_parallel_flag, self_loop=use_self_loop, bf16_training=bf16_training)
        self.layers = nn.ModuleList(
            [HET_RGATLayer(h_dim, h_dim, num_etypes, num_heads, activation=F.relu, dropout=dropout, **flags)
             for _ in range(num_hidden_layers)])
        last_heads = num_heads if num_hidden_layers == 0 else 1  # models.py:469-472
        self.layers.append(HET_RGATLayer(h_dim, out_dim, num_etypes, last_heads,
                                         activation=F.relu if last_layer_act else None, **flags))

    def forward(self, g, h):
        for layer in self.layers:
            h = layer(g, h)
        return h


class HET_RGCNModel(nn.Module):
    """hrt/python/RGCN/RGCN.py:353-405 (full-graph, edge-parallel separate-COO layers)."""

    def __init__(self, num_rels, h_dim, out_dim, num_layers=1, num_bases=-1, dropout=0.0, compact_as_of_node_flag=False,
                 compact_direct_indexing_flag=False, keyed_dropout=False, regularizer="basis"):
        super().__init__()
        dims = [h_dim] * num_layers + [out_dim]
        self.layers = nn.ModuleList(
            [HET_EglRelGraphConv_EdgeParallel(dims[i], dims[i + 1], num_rels, num_bases, regularizer=regularizer,
                                              activation=F.relu if i + 1 < num_layers else None, dropout=dropout,
                                              compact_as_of_node_flag=compact_as_of_node_flag,
                                              compact_direct_indexing_flag=compact_direct_indexing_flag, keyed_dropout=keyed_dropout)
             for i in range(num_layers)])

    def forward(self, g, h, norm):
        for layer in self.layers:
            h = layer(g, h, norm)
        return h


class HET_HGTModel(nn.Module):
    """hrt/python/HGT/models.py:246-347 (stack of HET_HGTLayerHetero)."""

    def __init__(self, num_ntypes, num_rels, h_dim, out_dim, num_heads, num_layers=1, dropout=0.2,
                 multiply_among_weights_first_flag=False, hgt_fused_attn_score_flag=False, use_norm=False):
        super().__init__()
        dims = [h_dim] * num_layers + [out_dim]
        self.layers = nn.ModuleList([HET_HGTLayerHetero(num_ntypes, num_rels, dims[i], dims[i + 1], num_heads=num_heads,
                                                        dropout=dropout, hgt_fused_attn_score_flag=hgt_fused_attn_score_flag,
                                                        multiply_among_weights_first_flag=multiply_among_weights_first_flag,
                                                        use_norm=use_norm)
                                     for i in range(num_layers)])

    def forward(self, g, h):
        for layer in self.layers:
            h = layer(g, h)
        return h


def add_generic_RGNN_args(p: argparse.ArgumentParser, default_logfilename: str):
    """The reference's generic flags (RGNNUtils.py:575-679), same names and defaults."""
    p.add_argument("--logfile_enabled", action="store_true", help="enable logging to json")
    p.add_argument("--logfilename", type=str, default=default_logfilename)
    p.add_argument("-d", "--dataset", type=str, default="mag", help="mag | aifb (synthetic graphs of those shapes)")
    p.add_argument("--n_infeat", type=int, default=64)
    p.add_argument("--sparse_format", type=str, default="csr")
    p.add_argument("--sort_by_src", action="store_true")
    p.add_argument("--sort_by_etype", action="store_true")
    p.add_argument("--no_reindex_eid", action="store_true")
    p.add_argument("--num_classes", type=int, default=8)
    p.add_argument("--use_real_labels_and_features", action="store_true")
    p.add_argument("--compact_direct_indexing_flag", action="store_true", default=False)
    p.add_argument("--lr", type=float, default=0.01)
    p.add_argument("--num_heads", type=int, default=1)
    p.add_argument("-e", "--n_epochs", type=int, default=10)
    p.add_argument("--fanout", type=int, nargs="+", default=[25, 20])
    p.add_argument("--batch_size", type=int, default=1024)
    p.add_argument("--full_graph_training", action="store_true")
    p.add_argument("--num_layers", type=int, default=1)
    p.add_argument("--compact_as_of_node_flag", action="store_true")
    p.add_argument("--no_warm_up", action="store_true")
    p.add_argument("--runs", type=int, default=1)
    p.add_argument("--dropout", type=float, default=0.5)
    # model-specific flags of RGAT/train_dgl.py:20-40, HGT/train.py
    p.add_argument("--multiply_among_weights_first_flag", action="store_true")
    p.add_argument("--gat_edge_parallel_flag", action="store_true", default=True)
    p.add_argument("--n_bases", type=int, default=-1)
    # ours
    p.add_argument("--model", default="rgat", choices=["rgat", "rgcn", "hgt"])
    p.add_argument("--scale", type=float, default=1.0, help="shrink the synthetic graph")
    p.add_argument("--edges_npy", type=str, default=None, help="[3, E] int array (src, dst, etype) instead of -d")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--inference", action="store_true",
                   help="time evaluation instead of training: every epoch is one forward under torch.no_grad() with the model in "
                        "eval(); backward is logged as 0")
    p.add_argument("--bf16_training", action="store_true",
                   help="RGAT only: bf16 input features and layers built with bf16_training=True (het_amd/layers.py: bf16 rows, fp32 "
                        "parameters and sums); the loss is taken on the logits cast to fp32")
    p.add_argument("--use_norm", action="store_true",
                   help="HGT only: the per-node-type LayerNorm after every layer's output projection (het_amd/layers.py)")
    p.add_argument("--sparse_embed", action="store_true",
                   help="sampled mini-batches only: the embedding table gives a row-sparse gradient (HET_RelGraphEmbed(sparse=True)) and is "
                        "stepped by het_amd.optim.RowSparseAdam -- a lazy Adam: the moments of rows a batch does not touch do not decay; "
                        "the model's parameters keep the fused Adam")
    p.add_argument("--keyed_sampler", action="store_true",
                   help="sampled mini-batches only: NeighborSampler(method='keyed') -- the kept in-edges are a pure function of (seed, "
                        "draw, edge position) and the blocks are built by the library's kernels (het_amd/sampling.py)")
    p.add_argument("--keyed_dropout", action="store_true",
                   help="RGAT / RGCN only: every layer ends with one KeyedDropout pass (activation and dropout fused, the mask a pure "
                        "function of (seed, draw, position), nothing stored for the backward; het_amd/layers.py) -- a different sample "
                        "than nn.Dropout's for the same --seed, the same distribution")
    p.add_argument("--fused_loss", action="store_true",
                   help="the loss (and the evaluation's) from het_amd.layers.SoftmaxCrossEntropy on the logits as the model returns them: "
                        "one HIP pass forward, one backward, no log-softmax tensor kept, summed in a fixed order -- instead of the torch "
                        "expression on logits.float()")
    p.add_argument("--regularizer", choices=("basis", "bdd"), default="basis",
                   help="RGCN only: 'bdd' gives every relation --n_bases diagonal blocks of [in / n_bases, out / n_bases] instead of a "
                        "dense (or basis-composed) weight, as DGL's RelGraphConv(regularizer='bdd'); --n_bases must divide --n_infeat "
                        "and --num_classes (het_amd/layers.py; the native kernels serve block sides 4 .. 32 of widths 32 / 64 / 128)")
    p.add_argument("--link_prediction", action="store_true",
                   help="full-graph encoder only: train for link prediction instead of node classification -- a DistMult head on the "
                        "encoder's output, --batch_size positive edges per step drawn by key from the graph, --num_negatives keyed "
                        "corruptions of each, BCE-with-logits (het_amd/linkpred.py); unfiltered negatives: a corruption may be a true edge")
    p.add_argument("--num_negatives", type=int, default=1, help="--link_prediction: keyed corruptions per positive edge")
    p.add_argument("--eval_ranking", type=int, default=0, metavar="P",
                   help="--link_prediction: after the last epoch rank P keyed positive edges on both sides against every node of the "
                        "true node's type, filtered on the graph's own edges, and log MRR, mean rank and Hits@1/3/10 "
                        "(het_amd/linkpred.py distmult_rank; the filter serves evaluation only, training negatives stay unfiltered)")
    p.add_argument("--decoder", choices=("distmult", "complex"), default="distmult",
                   help="--link_prediction: the head that scores the triples -- distmult (symmetric in head and tail) or complex "
                        "(ComplEx: tells a triple from its reverse; --num_classes is the even row width, a multiple of 4 for the HIP "
                        "kernels; het_amd/linkpred.py ComplExDecoder)")


def load_graph(args) -> IntegratedCOO:
    if args.edges_npy:
        a = th.from_numpy(np.load(args.edges_npy).astype(np.int64))
        n, r = int(a[:2].max()) + 1, int(a[2].max()) + 1
        o = th.sort(a[2], stable=True).indices
        return IntegratedCOO(n, r, th.tensor([0, n]), a[0][o].contiguous(), a[1][o].contiguous(), a[2][o].contiguous(),
                             th.arange(a.shape[1]))
    if args.dataset in ("mag", "ogbn-mag"):
        return make_mag_like(scale=args.scale)
    if args.dataset == "aifb":
        return make_aifb_like()
    raise SystemExit(f"dataset {args.dataset!r}: only the synthetic 'mag' / 'aifb' shapes or --edges_npy are available (no DGL/OGB)")


def aggregate_times(ms):
    """RGNNUtils.py:336-345, 364-384: drop epochs < 3, then the first quarter of what is left; arithmetic mean."""
    kept = ms[3:] if len(ms) > 3 else ms
    kept = kept[len(kept) // 4:]
    return float(sum(kept) / len(kept)) if kept else float("nan")


class OptimizerPair:
    """The optimizers of one training step behind the two calls HET_RGNN_train makes (--sparse_embed: the fused Adam of the model's
    parameters and the RowSparseAdam of the embedding table)."""

    def __init__(self, *optimizers):
        self.optimizers = optimizers

    def zero_grad(self):
        for o in self.optimizers:
            o.zero_grad()

    def step(self):
        for o in self.optimizers:
            o.step()


def HET_RGNN_train(g, model, node_embed_layer, optimizer, labels, args, extra=(), batches=None):
    """``batches``: None for full-graph training, else a callable returning (blocks, seeds) per step -- the sampled
    mini-batch path (het_amd/sampling.py); sampling + per-batch layout building is timed separately."""
    from .sampling import one_shot_graphs, run_blocks
    prep_ms = []

    inference = getattr(args, "inference", False)
    bf16 = getattr(args, "bf16_training", False)  # (the features enter the model as bf16 rows, the logits leave it as fp32)
    # --sparse_embed (sampled blocks only): the layer hands out the block's rows, in the model's dtype, through one autograd node
    sparse_embed = getattr(args, "sparse_embed", False) and batches is not None
    loss_fn = None  # --fused_loss: one pass each way over the logits in their own dtype
    if getattr(args, "fused_loss", False):
        from .layers import SoftmaxCrossEntropy
        loss_fn = SoftmaxCrossEntropy()

    def one_eval(timed):
        # the evaluation pass of the reference's scripts (model.eval() + torch.no_grad()): same inputs, same event pair around
        # the model as the training step's forward; loss from the same expression, nothing after it
        with th.no_grad():
            node_embed = node_embed_layer()
            cur_labels = labels
            if batches is not None:
                th.cuda.synchronize()
                t0 = time.perf_counter()
                blocks, seeds = batches()
                th.cuda.synchronize()
                prep_ms.append((time.perf_counter() - t0) * 1e3)
                node_embed, cur_labels = node_embed[blocks[0].nodes], labels[seeds]
            if bf16:
                node_embed = node_embed.to(th.bfloat16)
            th.cuda.synchronize()
            ev = [th.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            with (one_shot_graphs(blocks) if batches is not None else contextlib.nullcontext()):
                if batches is None:
                    logits = model(g, node_embed, *extra)
                else:
                    logits = run_blocks(model.layers, blocks, node_embed, extra[0] if extra else None)
                ev[1].record()
                if loss_fn is not None:
                    loss = loss_fn(logits, cur_labels)
                else:
                    logits = logits.float()
                    loss = -logits.log_softmax(dim=-1).gather(1, cur_labels.view(-1, 1)).mean()
            th.cuda.synchronize()
        return (ev[0].elapsed_time(ev[1]), 0.0, float(loss)) if timed else None

    def one_step(timed):
        if inference:
            return one_eval(timed)
        optimizer.zero_grad()
        node_embed = None if sparse_embed else node_embed_layer()
        cur_labels = labels
        if batches is not None:
            th.cuda.synchronize()
            t0 = time.perf_counter()
            blocks, seeds = batches()
            th.cuda.synchronize()
            prep_ms.append((time.perf_counter() - t0) * 1e3)
            if sparse_embed:
                node_embed = node_embed_layer(blocks[0].nodes, dtype=th.bfloat16 if bf16 else None)
            else:
                node_embed = node_embed[blocks[0].nodes]
            cur_labels = labels[seeds]
        if bf16 and not sparse_embed:
            node_embed = node_embed.to(th.bfloat16)
        th.cuda.synchronize()
        ev = [th.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        with (one_shot_graphs(blocks) if batches is not None else contextlib.nullcontext()):
            if batches is None:
                logits = model(g, node_embed, *extra)
            else:
                logits = run_blocks(model.layers, blocks, node_embed, extra[0] if extra else None)
            ev[1].record()
            logits = logits if loss_fn is not None else logits.float()
            # = F.nll_loss(logits.log_softmax(dim=-1), labels) (RGNNUtils.py:301-302), written as gather + mean: torch's 2-d
            # nll_loss kernels reduce 1.9 M rows in ONE workgroup on ROCm (4.6 ms forward, 3.0 ms backward on ogbn-mag --
            # more than the layer's own backward inside the protocol's "backward" figure)
            if loss_fn is not None:
                loss = loss_fn(logits, cur_labels)
            else:
                loss = -logits.log_softmax(dim=-1).gather(1, cur_labels.view(-1, 1)).mean()
            ev[2].record()
            loss.backward()
        optimizer.step()  # the reference times the optimizer inside "backward" (RGNNUtils.py:304-311)
        ev[3].record()
        th.cuda.synchronize()
        return (ev[0].elapsed_time(ev[1]), ev[2].elapsed_time(ev[3]), float(loss.detach())) if timed else None

    model.train(not inference)
    node_embed_layer.train(not inference)
    if not args.no_warm_up:
        for _ in range(5):
            one_step(False)
    fwd, bwd, losses = [], [], []
    for epoch in range(args.n_epochs):
        f, b, l = one_step(True)
        fwd.append(f); bwd.append(b); losses.append(l)
        print(f"Epoch {epoch:02d} | forward {f:.3f} ms | backward {b:.3f} ms | loss {l:.4f}")
    HET_RGNN_train.last_prep_ms = prep_ms
    return fwd, bwd, losses


def HET_linkpred_train(g, model, node_embed_layer, decoder, optimizer, args, extra=()):
    """--link_prediction: the full-graph encoder followed by a DistMult head (het_amd/linkpred.py).  Per step: h = model(g, embed()),
    --batch_size positive edges and --num_negatives corruptions of each, keyed by (--seed, draw = 2 step and 2 step + 1), scores,
    BCE-with-logits, backward, optimizer.  The event pairs are those of HET_RGNN_train: "forward" is the encoder; the batch, the
    decoder and the loss count inside "backward", with the optimizer."""
    from .linkpred import keyed_corruptions, keyed_positive_edges, link_prediction_loss
    N = g.get_num_nodes()
    offsets = g.get_original_node_type_offsets()
    offsets = None if offsets is None or offsets.numel() <= 2 else offsets
    steps = [0]

    def one_step(timed):
        step = steps[0]
        steps[0] += 1
        optimizer.zero_grad()
        node_embed = node_embed_layer()
        th.cuda.synchronize()
        ev = [th.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        h = model(g, node_embed, *extra)
        ev[1].record()
        ev[2].record()
        src, rel, dst = keyed_positive_edges(g, args.batch_size, seed=args.seed, draw=2 * step)
        s, r, o = keyed_corruptions(src, rel, dst, args.num_negatives, seed=args.seed, draw=2 * step + 1, node_type_offsets=offsets,
                                    num_nodes=N)
        loss = link_prediction_loss(decoder(h, s, r, o), args.batch_size)
        loss.backward()
        optimizer.step()
        ev[3].record()
        th.cuda.synchronize()
        return (ev[0].elapsed_time(ev[1]), ev[2].elapsed_time(ev[3]), float(loss.detach())) if timed else None

    model.train(True)
    node_embed_layer.train(True)
    decoder.train(True)
    if not args.no_warm_up:
        for _ in range(5):
            one_step(False)
    fwd, bwd, losses = [], [], []
    for epoch in range(args.n_epochs):
        f, b, l = one_step(True)
        fwd.append(f); bwd.append(b); losses.append(l)
        print(f"Epoch {epoch:02d} | forward {f:.3f} ms | backward {b:.3f} ms | loss {l:.4f}")
    return fwd, bwd, losses


RANKING_DRAW = -1  # the draw of the evaluation's positives: training uses the draws 2 step and 2 step + 1, all >= 0


def HET_linkpred_evaluate(g, model, node_embed_layer, decoder, args, extra=()):
    """--eval_ranking P: the encoder once under no_grad in evaluation mode, P positive edges keyed by (--seed, RANKING_DRAW) -- a draw
    no training step uses --, both sides ranked against the nodes of the true node's type, filtered on the graph's own edges
    (het_amd/linkpred.py).  Returns {mrr, mean_rank, hits@1, hits@3, hits@10, queries, ms}; ms is the ranking call alone (the pair
    plan included), between two events."""
    from .linkpred import FilterIndex, keyed_positive_edges, ranking_metrics
    offsets = g.get_original_node_type_offsets()
    offsets = None if offsets is None or offsets.numel() <= 2 else offsets
    was = model.training, node_embed_layer.training, decoder.training
    model.train(False)
    node_embed_layer.train(False)
    decoder.train(False)
    with th.no_grad():
        h = model(g, node_embed_layer(), *extra)
        src, rel, dst = keyed_positive_edges(g, args.eval_ranking, seed=args.seed, draw=RANKING_DRAW)
        filt = FilterIndex.from_graph(g)
        ev = [th.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        res = decoder.rank(h, src, rel, dst, sides="both", filter=filt, node_type_offsets=offsets)
        ev[1].record()
        th.cuda.synchronize()
        out = ranking_metrics(res, ks=(1, 3, 10))
    out["ms"] = round(ev[0].elapsed_time(ev[1]), 4)
    model.train(was[0])
    node_embed_layer.train(was[1])
    decoder.train(was[2])
    print("Ranking | " + " | ".join(f"{k} {v:.4f}" if isinstance(v, float) else f"{k} {v}" for k, v in out.items()))
    return out


def main(argv=None):
    p = argparse.ArgumentParser(description="HET RGAT / RGCN / HGT benchmark driver on het_amd (MI355X)")
    add_generic_RGNN_args(p, "het_amd_train.json")
    args = p.parse_args(argv)
    dev = th.device("cuda")
    if args.bf16_training and args.model != "rgat":
        raise SystemExit("--bf16_training is an option of the RGAT layer (RGCN and HGT train in bf16 on a bf16 input as they are)")
    if args.use_norm and args.model != "hgt":
        raise SystemExit("--use_norm is an option of the HGT layer")
    if args.keyed_dropout and args.model == "hgt":
        raise SystemExit("--keyed_dropout is an option of the RGAT and RGCN layers (the HGT layer applies no dropout)")
    if args.regularizer != "basis" and args.model != "rgcn":
        raise SystemExit("--regularizer is an option of the RGCN layer: add --model rgcn")
    if args.regularizer == "bdd" and (args.n_bases < 1 or args.n_infeat % args.n_bases or args.num_classes % args.n_bases):
        raise SystemExit("--regularizer bdd needs --n_bases >= 1 that divides --n_infeat and --num_classes")
    if args.sparse_embed and args.full_graph_training:
        raise SystemExit("--sparse_embed is an option of the sampled mini-batch path: --full_graph_training reads every row of the table")
    if args.sparse_embed and args.inference:
        raise SystemExit("--sparse_embed is an option of training: --inference takes no optimizer step")
    if args.keyed_sampler and args.full_graph_training:
        raise SystemExit("--keyed_sampler is an option of the sampled mini-batch path: --full_graph_training samples nothing")
    if args.link_prediction and not args.full_graph_training:
        raise SystemExit("--link_prediction runs the full-graph encoder: add --full_graph_training (edge-seeded sampled blocks are not built)")
    if args.link_prediction and args.inference:
        raise SystemExit("--link_prediction is an option of training: --inference scores no triples")
    if args.link_prediction and args.num_negatives < 0:
        raise SystemExit("--num_negatives is at least 0")
    if args.decoder != "distmult" and not args.link_prediction:
        raise SystemExit("--decoder chooses the head of a link-prediction run: add --link_prediction")
    if args.decoder == "complex" and args.num_classes % 2:
        raise SystemExit("--decoder complex needs an even --num_classes (pairs of a real and an imaginary column; a multiple of 4 for "
                         "the HIP kernels)")
    if args.eval_ranking and not args.link_prediction:
        raise SystemExit("--eval_ranking ranks the triples of a link-prediction run: add --link_prediction")
    if args.eval_ranking < 0 or args.eval_ranking >= 2 ** 29:
        raise SystemExit("--eval_ranking is a number of positive edges, at least 0 and fewer than 2^29")
    th.manual_seed(args.seed)
    coo = load_graph(args)
    for f in ("row", "col", "rel", "eids", "node_type_offsets"):
        setattr(coo, f, getattr(coo, f).to(dev))
    t0 = time.perf_counter()
    g = HetGraph.from_integrated_coo(coo, full=True)
    th.cuda.synchronize()
    layout_ms = (time.perf_counter() - t0) * 1e3
    N, E, R = g.get_num_nodes(), g.get_num_edges(), g.get_num_rels()
    print("Graph stats: ", E, N, R)
    embed = HET_RelGraphEmbed(N, args.n_infeat, sparse=args.sparse_embed).to(dev)
    extra = ()
    if args.model == "rgat":
        model = HET_RGATModel(R, args.n_infeat, args.num_classes, args.num_heads, num_hidden_layers=args.num_layers - 1,
                              dropout=args.dropout, use_self_loop=True,
                              compact_as_of_node_flag=args.compact_as_of_node_flag,
                              compact_direct_indexing_flag=args.compact_direct_indexing_flag,
                              multiply_among_weights_first_flag=args.multiply_among_weights_first_flag,
                              gat_edge_parallel_flag=args.gat_edge_parallel_flag, bf16_training=args.bf16_training,
                              keyed_dropout=args.keyed_dropout)
    elif args.model == "rgcn":
        model = HET_RGCNModel(R, args.n_infeat, args.num_classes, num_layers=args.num_layers, num_bases=args.n_bases,
                              dropout=args.dropout, compact_as_of_node_flag=args.compact_as_of_node_flag,
                              compact_direct_indexing_flag=args.compact_direct_indexing_flag, keyed_dropout=args.keyed_dropout,
                              regularizer=args.regularizer)
        extra = (th.rand(E, 1, device=dev),)  # edge norm as RGCN.py:527-530
    else:
        model = HET_HGTModel(g.get_num_ntypes(), R, args.n_infeat, args.num_classes, args.num_heads,
                             num_layers=args.num_layers, dropout=args.dropout,
                             multiply_among_weights_first_flag=args.multiply_among_weights_first_flag,
                             hgt_fused_attn_score_flag=getattr(args, "hgt_fused_attn_score_flag", False), use_norm=args.use_norm)
    model = model.to(dev)
    labels = th.randint(0, args.num_classes, (N,), device=dev)  # random labels as train_dgl.py:132-148
    params = list(model.parameters()) + ([] if args.sparse_embed else list(embed.parameters()))
    decoder = None
    if args.link_prediction:  # the head scores the encoder's output rows: their width is --num_classes
        from .linkpred import ComplExDecoder, DistMultDecoder
        decoder = (ComplExDecoder if args.decoder == "complex" else DistMultDecoder)(R, args.num_classes).to(dev)
        params += list(decoder.parameters())
    try:  # one kernel per step over all parameters (the [N, in] embedding table dominates); same update rule
        optimizer = th.optim.Adam(params, lr=args.lr, fused=True)
    except (RuntimeError, TypeError):
        optimizer = th.optim.Adam(params, lr=args.lr)
    if args.sparse_embed:
        from .optim import RowSparseAdam
        optimizer = OptimizerPair(optimizer, RowSparseAdam(embed.parameters(), lr=args.lr))
    batches = None
    if not args.full_graph_training:  # sampled blocks, one batch of --batch_size seeds per step ("epoch" = one step here)
        from .sampling import NeighborSampler
        fan = list(args.fanout)[: args.num_layers] + [args.fanout[-1]] * max(0, args.num_layers - len(args.fanout))
        sampler = NeighborSampler(g, fan, seed=args.seed,
                                  full_layouts=bool(args.compact_as_of_node_flag) or not args.gat_edge_parallel_flag
                                  or args.model == "hgt", by_type=args.model == "hgt",
                                  method="keyed" if args.keyed_sampler else "sort")
        gen = th.Generator(device=dev)
        gen.manual_seed(args.seed)

        def batches():
            seeds = th.randperm(N, device=dev, generator=gen)[: args.batch_size]
            blocks = sampler.sample_blocks(seeds)
            return blocks, blocks[-1].nodes[: blocks[-1].num_dst]  # the seeds in block order (by node type for HGT)
    if args.link_prediction:
        HET_RGNN_train.last_prep_ms = []
        fwd, bwd, losses = HET_linkpred_train(g, model, embed, decoder, optimizer, args, extra)
        ranking = HET_linkpred_evaluate(g, model, embed, decoder, args, extra) if args.eval_ranking else None
    else:
        fwd, bwd, losses = HET_RGNN_train(g, model, embed, optimizer, labels, args, extra, batches)
    res = {"model": args.model, "dataset": args.edges_npy or args.dataset, "num_nodes": N, "num_edges": E, "num_rels": R,
           "mean_forward_ms": round(aggregate_times(fwd), 4), "mean_backward_ms": round(aggregate_times(bwd), 4),
           "layout_build_ms": round(layout_ms, 1), "final_loss": losses[-1] if losses else None,
           "minibatch_sample_and_layout_ms": (round(aggregate_times(HET_RGNN_train.last_prep_ms), 3)
                                              if HET_RGNN_train.last_prep_ms else None),
           "peak_memory_GB": round(th.cuda.max_memory_allocated() / 2**30, 3), "args": vars(args)}
    if args.inference:
        res["mode"] = "inference"
    else:
        del res["args"]["inference"]  # (a training run's log line is what it was before the flag existed)
    if args.bf16_training:
        res["activations"] = "bf16"
    else:
        del res["args"]["bf16_training"]
    if not args.use_norm:
        del res["args"]["use_norm"]
    if args.sparse_embed:
        res["sparse_embed"] = True
    else:
        del res["args"]["sparse_embed"]
    if args.keyed_sampler:
        res["sampler"] = "keyed"
    else:
        del res["args"]["keyed_sampler"]
    if args.keyed_dropout:
        res["dropout"] = "keyed"
    else:
        del res["args"]["keyed_dropout"]
    if args.fused_loss:
        res["loss"] = "fused"
    else:
        del res["args"]["fused_loss"]
    if args.regularizer == "basis":
        del res["args"]["regularizer"]
    if args.link_prediction:
        res["task"] = "link_prediction"
    else:
        del res["args"]["link_prediction"]
        del res["args"]["num_negatives"]
    if args.decoder == "distmult":
        del res["args"]["decoder"]
    if args.eval_ranking:
        res["ranking"] = ranking
    else:
        del res["args"]["eval_ranking"]
    res["million_edges_per_s"] = round(E / ((res["mean_forward_ms"] + res["mean_backward_ms"]) * 1e-3) / 1e6, 2)
    print(json.dumps(res))
    if args.logfile_enabled:
        with open(args.logfilename, "a") as f:
            f.write(json.dumps(res) + "\n")
    return res


if __name__ == "__main__":
    main()
