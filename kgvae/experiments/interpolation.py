"""Latent-space analysis:  python -m kgvae.experiments.interpolation --config configs/<file>.yaml [--checkpoint-dir DIR]

Loads a SAIL / t-SAIL checkpoint written by kgvae.experiments.train and measures how the decoded graph changes along walks
through the latent space: a random neighbourhood of one point, a line walk, a Jaccard smoothness score over several walks
and the flip rate / basin length of small steps.  Same command line, function names, arguments, return values and printed
summaries as the reference's script of the same path (overlap ratios, Jaccard, flip rate, basin lengths with its trailing
basin rule); the two functions that only print there also return what they print.

What is different is how the points are decoded.  The reference decodes every point of every walk on its own
(`decode_latent(z.unsqueeze(0))`: its beam is shared by a batch, so only a batch of one gives a latent its own beam) -- 600
decodes for one flip rate.  Here every function first draws all its random vectors in the reference's order (z0, then the
directions, per anchor), builds all points of all walks, decodes them in ONE `decode_latent(..., per_latent=True)` call
(Engine.beam_decode_rows: every latent its own beam and its own stop) and computes its statistics on the host.  The point
construction (line_points) and the statistics (flip_stats, jaccard_stats, overlap_stats) take latents and decoded triple
sets, so they can be used on latents of one's own.

`--device-stats` (device_stats=True of the smoothness score and the flip rate): the decoded tokens stay on the device, the
graphs are compared there (ark_amd.graphs: canonical graphs and ark_graph_pair_stats over every walk's pairs) and only three
integers per pair come back; the returned numbers are the same.

Out of scope: the reference's two wd-movies figure functions (t-SNE of encoded test graphs, networkx drawings of an
interpolation).  They need sklearn, matplotlib, networkx and the IntelliGraphs files, none of which this package depends on.
`wandb` is optional, as in kgvae.experiments.train."""
import argparse
import os

import torch
import torch.nn as nn
import yaml

from kgvae.model.models import SAIL
from kgvae.model.utils import ints_to_labels, seq_to_triples

EPSILONS = [0.02, 0.05, 0.07, 0.1, 0.12, 0.15, 0.17, 0.2]


def jaccard(a: set, b: set) -> float:
    """|a & b| / |a | b|; 1 when both sets are empty, 0 when one is"""
    if not a and not b:
        return 1.0
    if not a or not b:
        return 0.0
    return len(a & b) / len(a | b)


# ---------------------------------------------------------------------------------------------------- points and statistics
def _unwrap(model):
    return model.module if isinstance(model, nn.DataParallel) else model


def _codec(model):
    c = model.config
    return c["seq_len"], c["special_tokens"], c["ENT_BASE"], c["REL_BASE"]


def unit(v):
    """v / |v| along the last axis"""
    return v / v.norm(dim=-1, keepdim=True).clamp_min(1e-12)


def line_points(z0, direction, steps, epsilon):
    """[steps + 1, Z]: z0 + (s * epsilon) * direction for s = 0 .. steps (point 0 is z0 itself)"""
    return torch.stack([z0 + (s * epsilon) * direction for s in range(steps + 1)])


def decode_graphs(model, zs, seq_len, special_tokens, entity_base_idx, relation_base_idx, beam=3):
    """one list of (h, r, t) id triples per latent of zs [n, Z]: ONE per-latent decode call"""
    return _unwrap(model).decode_latent(zs, seq_len, special_tokens, seq_to_triples, entity_base_idx, relation_base_idx,
                                        beam=beam, per_latent=True)


def as_triple_set(graph) -> set:
    return set(tuple(map(int, t)) for t in graph)


def decode_points(model, zs, seq_len, special_tokens, entity_base_idx, relation_base_idx, beam=3):
    """one set of (h, r, t) id triples per latent of zs [n, Z]: ONE per-latent decode call"""
    return [as_triple_set(g) for g in decode_graphs(model, zs, seq_len, special_tokens, entity_base_idx, relation_base_idx, beam)]


def decode_to_triple_set(model_unwrapped, z: torch.Tensor, seq_len: int, special_tokens: dict, entity_base_idx: int,
                         relation_base_idx: int, beam: int = 3) -> set:
    """the set of (h, r, t) id triples decoded from ONE latent z [Z]"""
    return decode_points(model_unwrapped, z.unsqueeze(0), seq_len, special_tokens, entity_base_idx, relation_base_idx, beam)[0]


def flip_stats(sets):
    """one walk (sets[0] the anchor) -> (number of steps whose set differs from the previous one's, basin lengths).  A basin is
    a run of consecutive points with the same set; it is recorded when a flip ends it, and the trailing one when the last
    step was no flip"""
    flips, basins, run, last_flip = 0, [], 1, False
    for prev, cur in zip(sets, sets[1:]):
        if cur != prev:
            flips += 1
            basins.append(run)
            run, last_flip = 1, True
        else:
            run, last_flip = run + 1, False
    if not last_flip and run > 0:
        basins.append(run)
    return flips, basins


def jaccard_stats(sets):
    """one walk (sets[0] the anchor) -> per step (jaccard(step, previous), jaccard(step, anchor))"""
    return [(jaccard(cur, prev), jaccard(cur, sets[0])) for prev, cur in zip(sets, sets[1:])]


def overlap_stats(graphs):
    """one walk of label-triple lists (graphs[0] the anchor) -> per step (|previous & step| / max(1, |previous|),
    |anchor & step| / max(1, |anchor|)), the lengths being those of the lists"""
    out = []
    denom_anchor = max(1, len(graphs[0]))
    for prev, cur in zip(graphs, graphs[1:]):
        out.append((len(set(prev) & set(cur)) / max(1, len(prev)), len(set(graphs[0]) & set(cur)) / denom_anchor))
    return out


def draw_walks(latent_dim, n_anchors, n_dirs, device):
    """the reference's draws, in its order: per anchor z0, then its n_dirs directions (normalised) -> [(z0, direction)]"""
    walks = []
    for _ in range(n_anchors):
        z0 = torch.randn(latent_dim, device=device)
        for _ in range(n_dirs):
            walks.append((z0, unit(torch.randn(latent_dim, device=device))))
    return walks


def decode_walks(model, walks, steps, epsilon, beam):
    """all points of all walks in ONE decode call -> per walk its steps + 1 triple sets (the first is the anchor's)"""
    model_unwrapped = _unwrap(model)
    pts = torch.cat([line_points(z0, direction, steps, epsilon) for z0, direction in walks])
    sets = decode_points(model_unwrapped, pts, *_codec(model_unwrapped), beam=beam)
    return [sets[w * (steps + 1):(w + 1) * (steps + 1)] for w in range(len(walks))]


def walk_pair_counts(model, walks, steps, epsilon, beam):
    """the device form of decode_walks: all points of all walks in ONE per-latent decode whose tokens stay on the device
    (SAIL.decode_latent_tokens), canonical graphs (ark_amd.graphs.canon) and ONE pair_stats call over every walk's
    (step, previous) and (step, anchor) pairs.  -> per walk, per step ((inter, d_step, d_previous), (inter, d_step,
    d_anchor)): distinct triples in common and on either side, as Python ints"""
    from ark_amd import graphs
    model_unwrapped = _unwrap(model)
    seq_len, special_tokens, _, _ = _codec(model_unwrapped)
    pts = torch.cat([line_points(z0, direction, steps, epsilon) for z0, direction in walks])
    toks, lens = model_unwrapped.decode_latent_tokens(pts, seq_len, special_tokens, beam=beam, per_latent=True)
    batch = graphs.canon(toks, lens, eos=special_tokens["EOS"], vocab=model_unwrapped.config["vocab_size"])
    ia, ib = graphs.walk_pairs(len(walks), steps)
    inter, da, db = (x.tolist() for x in graphs.pair_stats(batch, ia, ib))
    trip = list(zip(inter, da, db))
    half = len(walks) * steps
    return [list(zip(trip[w * steps:(w + 1) * steps], trip[half + w * steps:half + (w + 1) * steps])) for w in range(len(walks))]


# ---------------------------------------------------------------------------------------------------- checkpoint
def load_model(checkpoint_dir, dataset, model_type, epoch=None, device=None):
    """-> (model in eval mode, its config, the checkpoint's path, vocabularies, dataset_meta) from
    <dataset>_<model_type>_best_model.pt, or ..._checkpoint_epoch_<epoch>.pt when an epoch is given"""
    device = device or ("cuda" if torch.cuda.is_available() else "cpu")
    tail = "best_model.pt" if epoch is None else f"checkpoint_epoch_{epoch}.pt"
    ckpt_path = os.path.join(checkpoint_dir, f"{dataset}_{model_type}_{tail}")
    ckpt = torch.load(ckpt_path, map_location=device, weights_only=False)
    config = ckpt["config"]
    for key in ("ablation_encoder", "ablation_decoder"):
        val = config.get(key)
        if not val or str(val).lower() == "none":
            config[key] = "Transformer"
    state = ckpt["model_state_dict"]
    if any(k.startswith("module.") for k in state):
        state = {k.replace("module.", "", 1): v for k, v in state.items()}
    if model_type not in ("SAIL", "t-SAIL"):
        raise ValueError(f"Unknown model_type: {model_type}")
    model = SAIL(config).to(device)
    model.load_state_dict(state)
    model.eval()
    return model, config, ckpt_path, ckpt.get("vocabs", None), ckpt.get("dataset_meta", None)


# ---------------------------------------------------------------------------------------------------- the four analyses
def _print_graph(graph):
    for h, r, t in graph:
        print(f"({h}, {r}, {t})")


@torch.no_grad()
def random_steps_latent_autoreg(model, i2e, i2r, n_directions=20, epsilon=1.2, device=None):
    """a random point z0 and n_directions points at distance epsilon from it in random directions: prints every decoded graph
    and how many of the reference graph's triples it shares.  Two decode calls: z0, then all perturbed points"""
    model_unwrapped = _unwrap(model)
    seq_len, special_tokens, entity_base_idx, relation_base_idx = _codec(model_unwrapped)
    latent_dim = model_unwrapped.config["d_latent"]
    if device is None:
        device = next(model_unwrapped.parameters()).device
    z0 = torch.randn(latent_dim, device=device)
    directions = unit(torch.randn(n_directions, latent_dim, device=device))
    perturbed_zs = z0.unsqueeze(0) + epsilon * directions
    codec = (seq_len, special_tokens, entity_base_idx, relation_base_idx)
    ref_triples = ints_to_labels(decode_graphs(model_unwrapped, z0.unsqueeze(0), *codec, beam=3), i2e, i2r)[0]
    decoded_triples = ints_to_labels(decode_graphs(model_unwrapped, perturbed_zs, *codec, beam=3), i2e, i2r)
    print("\n=== Local Latent Neighborhood Exploration ===")
    print("\n--- Reference Graph (z₀) ---")
    _print_graph(ref_triples)
    overlaps = []
    denom = max(1, len(ref_triples))
    for i, graph in enumerate(decoded_triples):
        print(f"\n--- Perturbed z #{i+1} ---")
        _print_graph(graph)
        overlaps.append(len(set(ref_triples) & set(graph)))
        print(f"# Overlapping triples with z₀: {overlaps[-1]} / {denom}")
    return overlaps, denom


@torch.no_grad()
def smoothness_line_check_autoreg(model, i2e, i2r, steps: int = 10, epsilon: float = 0.1, device: str = None, beam: int = 3):
    """`steps` steps of size epsilon from a random point along a random unit direction: prints every decoded graph with its
    overlap with the previous step's (local smoothness) and with the anchor's (global overlap), then the two averages"""
    model_unwrapped = _unwrap(model)
    latent_dim = model_unwrapped.config["d_latent"]
    if device is None:
        device = next(model_unwrapped.parameters()).device
    z0 = torch.randn(latent_dim, device=device)
    direction = unit(torch.randn(latent_dim, device=device))
    pts = line_points(z0, direction, steps, epsilon)
    graphs = ints_to_labels(decode_graphs(model_unwrapped, pts, *_codec(model_unwrapped), beam=beam), i2e, i2r)
    print("\n=== Latent Smoothness Line Walk ===")
    print(f"Steps: {steps} | step size ε = {epsilon}")
    print("\n--- Anchor (z₀) ---")
    _print_graph(graphs[0])
    total_local = total_global = 0.0
    for s, (local_overlap, global_overlap) in enumerate(overlap_stats(graphs), start=1):
        total_local += local_overlap
        total_global += global_overlap
        print(f"\n--- Step {s}: z = z₀ + {s}·ε·direction ---")
        _print_graph(graphs[s])
        print(f"Local smoothness (vs step {s-1}): {local_overlap:.2f}")
        print(f"Global overlap (vs anchor)     : {global_overlap:.2f}")
    print("\n=== Summary ===")
    print(f"Avg local smoothness over {steps} steps: {total_local/steps:.2f}")
    print(f"Avg global overlap over {steps} steps : {total_global/steps:.2f}")
    return total_local / steps, total_global / steps


@torch.no_grad()
def latent_smoothness_score_autoreg(model, steps: int = 10, epsilon: float = 0.1, n_anchors: int = 3, n_dirs: int = 3, beam: int = 3,
                                    device: str = None, device_stats: bool = False):
    """-> (average Jaccard between consecutive steps, average Jaccard between each step and its anchor) over n_anchors x
    n_dirs walks of `steps` steps.  device_stats: the decoded tokens stay on the device and the set sizes come from
    ark_graph_pair_stats (walk_pair_counts); the same numbers"""
    model_unwrapped = _unwrap(model)
    if device is None:
        device = next(model_unwrapped.parameters()).device
    walks = draw_walks(model_unwrapped.config["d_latent"], n_anchors, n_dirs, device)
    total_local = total_global = 0.0
    count = 0
    if walks and steps > 0:
        if device_stats:
            from ark_amd.graphs import jaccard_stats_from_counts
            per_walk = [jaccard_stats_from_counts(*zip(*w)) for w in walk_pair_counts(model_unwrapped, walks, steps, epsilon, beam)]
        else:
            per_walk = [jaccard_stats(sets) for sets in decode_walks(model_unwrapped, walks, steps, epsilon, beam)]
        for stats in per_walk:
            for local, glob in stats:          # (summed step by step, in the reference's order)
                total_local += local
                total_global += glob
                count += 1
    avg_local = total_local / max(1, count)
    avg_global = total_global / max(1, count)
    print(f"\n[SMOOTHNESS SCORE] anchors={n_anchors}, dirs={n_dirs}, steps={steps}, ε={epsilon}")
    print(f"Avg local Jaccard : {avg_local:.3f}")
    print(f"Avg global Jaccard: {avg_global:.3f}")
    return avg_local, avg_global


@torch.no_grad()
def latent_flip_rate_autoreg(model, steps: int = 30, epsilon: float = 0.05, n_anchors: int = 5, n_dirs: int = 4, beam: int = 3,
                             device: str = None, device_stats: bool = False):
    """-> (fraction of steps that change the decoded graph, average number of consecutive points with the same graph) over
    n_anchors x n_dirs walks of `steps` steps.  device_stats: as in latent_smoothness_score_autoreg"""
    model_unwrapped = _unwrap(model)
    if device is None:
        device = next(model_unwrapped.parameters()).device
    walks = draw_walks(model_unwrapped.config["d_latent"], n_anchors, n_dirs, device)
    total_flips = total_steps = 0
    all_basin_lengths = []
    if walks:
        if device_stats and steps > 0:
            from ark_amd.graphs import flip_stats_from_equal, sets_equal
            per_walk = [flip_stats_from_equal([sets_equal(*prev) for prev, _ in w])
                        for w in walk_pair_counts(model_unwrapped, walks, steps, epsilon, beam)]
        else:
            per_walk = [flip_stats(sets) for sets in decode_walks(model_unwrapped, walks, steps, epsilon, beam)]
        for flips, basins in per_walk:
            total_flips += flips
            total_steps += steps
            all_basin_lengths += basins
    flip_rate = total_flips / max(1, total_steps)
    avg_basin = sum(all_basin_lengths) / max(1, len(all_basin_lengths))
    print(f"\n[FLIP RATE] anchors={n_anchors}, dirs={n_dirs}, steps={steps}, ε={epsilon}")
    print(f"Flip rate      : {flip_rate:.3f} (fraction of step transitions that change graph)")
    print(f"Avg basin len  : {avg_basin:.2f} steps")
    return flip_rate, avg_basin


# ---------------------------------------------------------------------------------------------------- command line
def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('--config', type=str, required=True, help='Path to config file')
    parser.add_argument('--checkpoint-dir', type=str, default='checkpoints')
    parser.add_argument('--wandb-project', type=str, default='submission', help='Weights & Biases project name')
    parser.add_argument('--wandb-entity', type=str, default=None, help='Weights & Biases entity')
    parser.add_argument('--directions', type=int, default=20)
    parser.add_argument('--epsilon', type=float, default=0.1)
    parser.add_argument('--epoch', type=int, default=None, help='If set, load that epoch; else load best')
    parser.add_argument('--device-stats', action='store_true',
                        help='smoothness score and flip rate from graph keys computed on the device (same numbers)')
    args = parser.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("kgvae.experiments.interpolation needs an AMD GPU: the model runs on hand-written gfx950 kernels only")
    with open(args.config, 'r') as f:
        config = yaml.safe_load(f)
    dataset = config['dataset']
    model_type = config.get('model_type', 'SAIL')
    device = 'cuda'
    beam = config.get("beam_width", 3)
    model, config, ckpt_path, vocabs, _ = load_model(checkpoint_dir=args.checkpoint_dir, dataset=dataset, model_type=model_type,
                                                     epoch=args.epoch, device=device)
    if vocabs is None:
        raise KeyError("Checkpoint missing 'vocabs'; retrain and save with vocabulary mappings.")
    missing = [k for k in ("i2e", "i2r") if vocabs.get(k) is None]
    if missing:
        raise KeyError(f"Checkpoint vocabulary missing keys: {missing}")
    i2e, i2r = vocabs["i2e"], vocabs["i2r"]
    try:
        import wandb
        wandb.init(project=args.wandb_project, entity=args.wandb_entity, config=config,
                   name=f"latent_interp_{config['dataset']}_{config.get('model_type', 'SAIL')}")
    except Exception:
        wandb = None
    kind = f"epoch {args.epoch}" if args.epoch is not None else "best"
    print(f"✅ Loaded {model_type} for {dataset} ({kind}) from {ckpt_path} on {device}")
    if dataset == "wd-movies":
        print("(the wd-movies t-SNE / networkx figures of the reference are not part of this package)")
    for e in EPSILONS:
        print("----------------------------------------------------------------------")
        print("epsilon value is:", e)
        print("----------------------------------------------------------------------")
        random_steps_latent_autoreg(model, i2e=i2e, i2r=i2r, n_directions=args.directions, epsilon=e, device=device)
        smoothness_line_check_autoreg(model, i2e=i2e, i2r=i2r, steps=10, epsilon=e, device=device, beam=beam)
        latent_smoothness_score_autoreg(model, steps=10, epsilon=e, n_anchors=3, n_dirs=3, beam=beam, device=device,
                                        device_stats=args.device_stats)
        latent_flip_rate_autoreg(model, steps=30, epsilon=e, n_anchors=5, n_dirs=4, beam=beam, device=device,
                                 device_stats=args.device_stats)
    if wandb is not None:
        wandb.finish()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
