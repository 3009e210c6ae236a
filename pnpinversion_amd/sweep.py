"""What the PIE-Bench sweep drivers (run_editing_*.py) share: the reference scripts' flags, the work list with its skip-if-exists resume,
the rank / device / weight start-up with its shutdown, and the panel save.  Host only; torch is imported where a function needs it.
A driver keeps its own flags, its pipeline, its edit functions and the order of its loop ("sweep drivers")."""
import contextlib
import json
import os
import random
import types

import numpy as np


def mask_decode(encoded_mask, image_shape=(512, 512)):
    """PIE-Bench run-length mask: [start0, len0, start1, len1, ...] over the flattened image; the border is forced to 1
    (run_editing_p2p.py:11-27)."""
    n = image_shape[0] * image_shape[1]
    mask = np.zeros(n)
    runs = np.asarray(encoded_mask, dtype=np.int64).reshape(-1, 2)
    for start, length in runs:
        mask[start:start + min(length, n - start)] = 1
    mask = mask.reshape(image_shape)
    mask[0, :] = mask[-1, :] = 1
    mask[:, 0] = mask[:, -1] = 1
    return mask


def setup_seed(seed=1234):
    import torch
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)
    np.random.seed(seed)
    random.seed(seed)


def add_sweep_args(ap, default_methods):
    """The reference scripts' five flags, --model_config and the weight flags; a driver adds its own after these."""
    from .checkpoint import add_weight_args
    ap.add_argument("--rerun_exist_images", action="store_true")
    ap.add_argument("--data_path", type=str, default="data")
    ap.add_argument("--output_path", type=str, default="output")
    ap.add_argument("--edit_category_list", nargs="+", type=str, default=[str(i) for i in range(10)])
    ap.add_argument("--edit_method_list", nargs="+", type=str, default=list(default_methods))
    ap.add_argument("--model_config", choices=("sd1", "small64"), default="sd1", help="small64: reduced-width test configuration")
    add_weight_args(ap)


def check_methods(ap, args, known):
    unknown = [m for m in args.edit_method_list if m not in known]
    if unknown:
        ap.error("unknown edit method(s) %s; this script runs %s" % (unknown, list(known)))


def clean_prompt(s):
    return s.replace("[", "").replace("]", "")


def read_mapping(args):
    with open(os.path.join(args.data_path, "mapping_file.json")) as f:
        return json.load(f)


def shard(args, instructions, rank=0, world=1):
    """This rank's share of the mapping file -> [(item, image_path)]: category filter, then round-robin over the ranks."""
    from .distributed import shard_items
    work = [v for v in instructions.values() if v["editing_type_id"] in args.edit_category_list]
    return [(item, os.path.join(args.data_path, "annotation_images", item["image_path"])) for item in shard_items(work, rank, world)]


def pending(args, image_path, out_dir, log=print, method=None):
    """Where the panel of image_path goes under --output_path/out_dir, or None (and the skip message) when it is there already and
    --rerun_exist_images is not set.  method: the name in the message where it is not the folder's."""
    out_path = image_path.replace(args.data_path, os.path.join(args.output_path, out_dir))
    if os.path.exists(out_path) and not args.rerun_exist_images:
        log(f"skip image [{image_path}] with [{method or out_dir}]")
        return None
    return out_path


def plan(args, instructions, out_dir, rank=0, world=1, log=print, method=None):
    """shard, then pending, for one method -> [(item, image_path, out_path)] still to edit on this rank, in the mapping file's order."""
    todo = []
    for item, image_path in shard(args, instructions, rank, world):
        out_path = pending(args, image_path, out_dir, log, method)
        if out_path is not None:
            todo.append((item, image_path, out_path))
    return todo


@contextlib.contextmanager
def session(args, configs, make_pipeline, load_weights=None):
    """One process per GPU (torch.distributed.run's RANK / WORLD_SIZE / LOCAL_RANK; a plain process is rank 0 of 1): environment, device,
    process group, weights on rank 0, make_pipeline(cfg, "cuda:<local_rank>", tokenizer), one RCCL broadcast of the weight arena; on a
    normal exit barrier + destroy_process_group.  configs: {--model_config value: ModelConfig}; load_weights(args, cfg, rank): default
    checkpoint.resolve_weights.  Yields .pipe .cfg .rank .world .local_rank .device."""
    import torch
    from .checkpoint import resolve_weights
    from .distributed import broadcast_weights, prepare_env
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    prepare_env()                      # dmabuf IPC + 127.0.0.1 rendezvous, before RCCL initialises
    torch.cuda.set_device(local_rank)
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    cfg = configs[args.model_config]
    unet_sd, vae_sd, clip_sd, tokenizer = (load_weights or resolve_weights)(args, cfg, rank)     # --checkpoint_dir | --synthetic_weights (loud)
    pipe = make_pipeline(cfg, "cuda:%d" % local_rank, tokenizer)
    if rank == 0:
        pipe.load_state_dict(unet_sd, vae_sd, clip_sd=clip_sd)
    if world > 1:
        bstats = {}
        broadcast_weights(pipe.engine, src=0, stats=bstats)
        if rank == 0:
            print("weight arena broadcast over RCCL: %.1f MB to %d ranks in %.1f ms" % (bstats["bytes"] / 1e6, bstats["ranks"], bstats["ms"]))
    yield types.SimpleNamespace(pipe=pipe, cfg=cfg, rank=rank, world=world, local_rank=local_rank, device=torch.device("cuda", local_rank))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def save_panel(panel, out_path):
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    panel.save(out_path)
    print("finish")
