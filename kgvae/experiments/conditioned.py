"""Conditioned generation:  python -m kgvae.experiments.conditioned --config configs/<file>.yaml [--checkpoints a.pt ...]

Loads checkpoints written by kgvae.experiments.train (any of SAIL / t-SAIL / ARK / t-ARK) and generates graphs whose FIRST
triple has a given relation and tail: positions 2 and 3 of every token sequence are forced to those two tokens, everything
else is decoded as usual (greedy by default, or with ARK.generate's sampling rules).  Same command line and function names
as the reference's script of the same path; the decoding itself runs on the engine's fused sampler
(Engine.sample_decode through SAIL.sample_latent / ARK.generate(sampler="fused")), which forces a token by returning it for
every row instead of masking the logits."""
import argparse
import copy
import glob
import os

import torch
import yaml

from kgvae.model.models import ARK, SAIL
from kgvae.model.utils import ints_to_labels, seq_to_triples

CONDITION_RELATION = "has_director"
CONDITION_OBJECT = "Tim Burton"
MODEL_TYPES = ("SAIL", "t-SAIL", "ARK", "t-ARK")


def load_checkpoint(path, device):
    """-> (config, model state dict, vocabularies) of a checkpoint of kgvae.experiments.train"""
    ckpt = torch.load(path, map_location=device, weights_only=False)
    return ckpt.get("config", {}), ckpt["model_state_dict"], ckpt.get("vocabs") or {}


def normalize_config(config, model_type_override=None):
    """-> (a copy of the config with `model_type` set to one of MODEL_TYPES, that model type)"""
    cfg = copy.deepcopy(dict(config))
    raw = model_type_override or cfg.get("model_type", "ARK")
    by_lower = {m.lower(): m for m in MODEL_TYPES}
    resolved = by_lower.get(str(raw).lower().replace("_", "-"))
    if resolved is None:
        raise ValueError(f"model_type {raw!r}: expected one of {MODEL_TYPES}")
    cfg["model_type"] = resolved
    return cfg, resolved


def build_model(config, state, device, model_type_override=None):
    """-> (model in eval mode on `device` with `state` loaded, its config, 'sail' or 'ark')"""
    cfg, resolved = normalize_config(config, model_type_override)
    kind = "sail" if resolved in ("SAIL", "t-SAIL") else "ark"
    model = (SAIL if kind == "sail" else ARK)(cfg).to(device)
    model.load_state_dict(state)
    model.eval()
    return model, cfg, kind


def ids_for_condition(vocabs, cfg, relation_label, object_label):
    """-> (token id of the relation, token id of the tail entity) in the decoder's vocabulary"""
    e2i, r2i = vocabs.get("e2i"), vocabs.get("r2i")
    if e2i is None or r2i is None:
        raise ValueError("the checkpoint holds no vocabularies (e2i / r2i)")
    if relation_label not in r2i:
        raise KeyError(f"relation {relation_label!r} is not in the checkpoint's vocabulary")
    if object_label not in e2i:
        raise KeyError(f"entity {object_label!r} is not in the checkpoint's vocabulary")
    return cfg["REL_BASE"] + int(r2i[relation_label]), cfg["ENT_BASE"] + int(e2i[object_label])


@torch.no_grad()
def conditional_generate(model, model_kind, cfg, forced_relation_id, forced_object_id, num_samples, device, sample=False,
                         temperature=1.0, top_p=0.0, top_k=0, seed=None):
    """num_samples token sequences [num_samples, seq_len] (on the CPU) with position 2 = forced_relation_id and
    position 3 = forced_object_id; SAIL kinds decode latents z ~ N(0, I) drawn from torch's generator on `device`"""
    forced = {2: int(forced_relation_id), 3: int(forced_object_id)}
    kw = dict(sample=sample, temperature=temperature, top_p=top_p, top_k=top_k, seed=seed, forced=forced)
    if model_kind == "sail":
        z = torch.randn(num_samples, cfg["d_latent"], device=device)
        seq = model.sample_latent(z, cfg["seq_len"], cfg["special_tokens"], **kw)
    else:
        seq = model.generate(cfg["seq_len"], cfg["special_tokens"], device=device, batch_size=num_samples, sampler="fused", **kw)
    return seq.cpu()


def to_labeled_triples(seqs, cfg, vocabs):
    """token sequences -> one list of (head, relation, tail) label triples per sequence"""
    graphs = [seq_to_triples(s, cfg["special_tokens"], cfg["ENT_BASE"], cfg["REL_BASE"]) for s in seqs]
    return ints_to_labels(graphs, vocabs["i2e"], vocabs["i2r"])


def discover_checkpoints(explicit, checkpoint_dir):
    if explicit:
        return list(explicit)
    return sorted(glob.glob(os.path.join(checkpoint_dir, "*.pt")))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=str, required=True, help="Path to config YAML file.")
    ap.add_argument("--checkpoints", nargs="+", default=None, help="One or more checkpoint files to load.")
    ap.add_argument("--checkpoint-dir", type=str, default="checkpoints", help="Fallback directory to scan for checkpoints.")
    ap.add_argument("--num-samples", type=int, default=4, help="Number of graphs to generate per checkpoint.")
    ap.add_argument("--device", type=str, default="cuda")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--relation", type=str, default=CONDITION_RELATION, help="Relation label to force in the first triple.")
    ap.add_argument("--tail", type=str, default=CONDITION_OBJECT, help="Tail entity label to force in the first triple.")
    ap.add_argument("--dataset", type=str, default=None, help="Dataset name used to filter checkpoints (overrides config).")
    ap.add_argument("--model-type", type=str, default=None, choices=list(MODEL_TYPES),
                    help="Override model type if checkpoint config is ambiguous.")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("kgvae.experiments.conditioned needs an AMD GPU: the model runs on hand-written gfx950 kernels only")
    with open(args.config, "r") as f:
        file_cfg = yaml.safe_load(f) or {}
    dataset = args.dataset or file_cfg.get("dataset")
    device = torch.device(args.device)
    torch.manual_seed(args.seed)
    paths = [p for p in discover_checkpoints(args.checkpoints, args.checkpoint_dir)
             if args.checkpoints or not dataset or os.path.basename(str(p)).startswith(str(dataset))]
    if not paths:
        print(f"no checkpoints found (directory {args.checkpoint_dir!r}, dataset {dataset!r})")
        return 1
    for path in paths:
        config, state, vocabs = load_checkpoint(path, device)
        model, cfg, kind = build_model({**file_cfg, **config}, state, device, args.model_type)
        rid, oid = ids_for_condition(vocabs, cfg, args.relation, args.tail)
        seqs = conditional_generate(model, kind, cfg, rid, oid, args.num_samples, device, seed=args.seed)
        print(f"\n{path} [{cfg['model_type']}]: first triple forced to (*, {args.relation}, {args.tail})")
        for i, graph in enumerate(to_labeled_triples(seqs, cfg, vocabs)):
            print(f"  sample {i}:")
            for h, r, t in graph:
                print(f"    ({h}, {r}, {t})")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
