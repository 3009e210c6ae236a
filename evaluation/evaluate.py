"""PIE-Bench evaluation table (the reference's evaluation/evaluate.py): one CSV row per benchmark image, one column per
(method folder, metric), for every column this library can compute:

  psnr* / mse* / ssim*      pnpinversion_amd.metrics (numpy restatements of the torchmetrics definitions)
  clip_similarity_*         on the device: pnpinversion_amd.clip_score.ClipScore (CLIP ViT-L/14 image tower + SD's own text tower)
  structure_distance*       on the device: pnpinversion_amd.structure_distance.StructureDistance (DINO ViT-B/8 key self-similarity)
  lpips*                    on the device: pnpinversion_amd.lpips.Lpips (SqueezeNet 1.1 features, torchmetrics >= 1.0's normalisation)

`structure_distance*` is not built without DINO weights (--dino_checkpoint or --synthetic_weights) and `lpips*` is not built without
LPIPS weights (--squeezenet_checkpoint with --lpips_checkpoint, or --synthetic_weights): asking for such a column ends the run with a
message naming it, before any file is opened.
Arguments, the method-folder table, the right-hand 512 crop of non-square panels, the "nan" cells of empty masks and the CSV layout are
the reference's.  The three CLIP columns of one (image, method) pair go to the device as ONE launch set (source image / source prompt,
target image / target prompt, masked target image / target prompt), and so do its three structure columns (whole, unedited part, edited
part: one tower pass over the six images) and its three LPIPS columns (likewise).

    python evaluation/evaluate.py --checkpoint_dir <SD-1.x dir> --clip_model_dir <clip-vit-large-patch14 dir> --dino_checkpoint <dino_vitbase8_pretrain.pth> \
                                  --squeezenet_checkpoint <squeezenet1_1-b8a52dc0.pth> --lpips_checkpoint <lpips squeeze.pth> [--metrics ...]
    python evaluation/evaluate.py --dino_checkpoint <dino_vitbase8_pretrain.pth> --metrics structure_distance psnr_unedit_part   # no CLIP weights needed
    python evaluation/evaluate.py --synthetic_weights ...        # seeded random towers: the numbers mean nothing, the plumbing runs
"""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PIXEL_METRICS = ("psnr", "mse", "ssim")
PARTS = ("", "_unedit_part", "_edit_part")
CLIP_METRICS = ("clip_similarity_source_image", "clip_similarity_target_image", "clip_similarity_target_image_edit_part")
STRUCT_METRICS = ("structure_distance", "structure_distance_unedit_part", "structure_distance_edit_part")
LPIPS_METRICS = ("lpips", "lpips_unedit_part", "lpips_edit_part")
DEFAULT_METRICS = ["structure_distance", "psnr_unedit_part", "lpips_unedit_part", "mse_unedit_part", "ssim_unedit_part"] + list(CLIP_METRICS)


def _folder_table():
    """table key -> folder of the method's panels.  Keys are "<table number>_<method>"; the folder is output/<method>/annotation_images,
    except that table 4 abbreviates null-text-inversion to null-text-inverse and tables 6 / 7 drop the "+p2p" of their folders."""
    guidance = ["directinversion+p2p_guidance_%s_%s" % (i, f) for i in ("0", "1", "25", "5", "75") for f in ("1", "5", "25", "75")]
    groups = [
        ("1", ["ddim+p2p", "null-text-inversion+p2p_a800", "null-text-inversion+p2p_3090", "negative-prompt-inversion+p2p", "stylediffusion+p2p",
               "directinversion+p2p", "ddim+masactrl", "directinversion+masactrl", "ddim+pix2pix-zero", "directinversion+pix2pix-zero", "ddim+pnp",
               "directinversion+pnp"]),
        ("2", ["instruct-pix2pix", "instruct-diffusion", "blended-latent-diffusion", "directinversion+p2p"]),
        ("3", guidance),
        ("4", ["null-text-inverse+p2p_a800", "null-text-inverse+p2p_3090", "null-text-inversion+proximal-guidance",
               "negative-prompt-inversion+proximal-guidance", "edit-friendly-inversion+p2p", "edict+direct_forward", "edict+p2p", "directinversion+p2p"]),
        ("5", ["ablation_directinversion_04+p2p", "ablation_directinversion_08+p2p", "ablation_null-latent-inversion+p2p_a800",
               "ablation_null-latent-inversion+p2p_3090", "ablation_null-text-inversion_single_branch+p2p_a800",
               "ablation_null-text-inversion_single_branch+p2p_3090"]),
        ("6", ["ablation_directinversion_interval_%d" % k for k in (2, 5, 10, 24, 49)]),
        ("7", ["ablation_directinversion_step_%d" % k for k in (20, 100, 500)]),
        ("8", ["ablation_directinversion_add-source+p2p", "ablation_directinversion_add-target+p2p"]),
    ]
    table = {}
    for num, methods in groups:
        for m in methods:
            folder = m.replace("null-text-inverse+", "null-text-inversion+") + ("+p2p" if num in ("6", "7") else "")
            table["%s_%s" % (num, m)] = "output/%s/annotation_images" % folder
    return table


all_tgt_image_folders = _folder_table()


def mask_decode(encoded_mask, image_shape=(512, 512)):
    """PIE-Bench's run-length mask ((start, length) pairs over the flattened image) -> float 0 / 1 [H, W]; the one-pixel border is set,
    as the reference does against annotation errors at the boundary"""
    length = image_shape[0] * image_shape[1]
    m = np.zeros(length)
    for start, run in zip(encoded_mask[0::2], encoded_mask[1::2]):
        m[start:start + min(run, length - start)] = 1
    m = m.reshape(image_shape[0], image_shape[1])
    m[0, :] = m[-1, :] = 1
    m[:, 0] = m[:, -1] = 1
    return m


def _split(metric):
    for part in ("_unedit_part", "_edit_part"):
        if metric.endswith(part):
            return metric[:-len(part)], part
    return metric, ""


def has_dino_weights(args):
    return bool(getattr(args, "dino_checkpoint", None) or getattr(args, "synthetic_weights", False))


def has_lpips_weights(args):
    return bool((getattr(args, "squeezenet_checkpoint", None) and getattr(args, "lpips_checkpoint", None)) or getattr(args, "synthetic_weights", False))


def check_metrics(metrics, dino=False, lpips=False):
    """dino / lpips: DINO / LPIPS weights (or a scorer) are at hand, so the structure_distance* / lpips* columns can be computed"""
    computable = [p + s for p in PIXEL_METRICS for s in PARTS] + list(CLIP_METRICS)
    for m in metrics:
        base, _ = _split(m)
        if m in LPIPS_METRICS:
            if not lpips:
                raise SystemExit("column %r is not built without LPIPS weights: pass --squeezenet_checkpoint <squeezenet1_1 state dict> with "
                                 "--lpips_checkpoint <the lpips package's squeeze.pth>, or --synthetic_weights for a seeded random network "
                                 "(computable without them: %s)" % (m, ", ".join(computable)))
            continue
        if m in STRUCT_METRICS:
            if not dino:
                raise SystemExit("column %r is not built without DINO weights: pass --dino_checkpoint <dino_vitbase8_pretrain.pth>, or "
                                 "--synthetic_weights for a seeded random ViT (computable without them: %s)" % (m, ", ".join(computable)))
            continue
        if m not in CLIP_METRICS and not (base in PIXEL_METRICS and m == base + _split(m)[1]):
            raise SystemExit("unknown metric column %r" % m)


class Calculator:
    """the reference's MetricsCalculator protocol for the columns that are built"""

    def __init__(self, scorer=None, struct_scorer=None, lpips_scorer=None):
        self.scorer, self.struct_scorer, self.lpips_scorer = scorer, struct_scorer, lpips_scorer

    def calculate_clip_similarity(self, img, txt, mask=None):
        from pnpinversion_amd import metrics
        return metrics.calculate_clip_similarity(img, txt, mask, scorer=self.scorer)

    def calculate_structure_distance(self, img_pred, img_gt, mask_pred=None, mask_gt=None):
        from pnpinversion_amd import metrics
        return metrics.calculate_structure_distance(img_pred, img_gt, mask_pred, mask_gt, scorer=self.struct_scorer)

    def calculate_lpips(self, img_pred, img_gt, mask_pred=None, mask_gt=None):
        from pnpinversion_amd import metrics
        return metrics.calculate_lpips(img_pred, img_gt, mask_pred, mask_gt, scorer=self.lpips_scorer)

    def __getattr__(self, name):
        from pnpinversion_amd import metrics
        if name in ("calculate_psnr", "calculate_mse", "calculate_ssim"):
            return getattr(metrics, name)
        raise AttributeError(name)


def calculate_metric(calc, metric, src_image, tgt_image, src_mask, tgt_mask, src_prompt, tgt_prompt):
    """one cell; "nan" where the mask leaves nothing to measure"""
    base, part = _split(metric)
    if metric in CLIP_METRICS:
        if metric == "clip_similarity_source_image":
            return calc.calculate_clip_similarity(src_image, src_prompt, None)
        if metric == "clip_similarity_target_image":
            return calc.calculate_clip_similarity(tgt_image, tgt_prompt, None)
        return "nan" if tgt_mask.sum() == 0 else calc.calculate_clip_similarity(tgt_image, tgt_prompt, tgt_mask)
    if (metric in STRUCT_METRICS and getattr(calc, "struct_scorer", None) is None) or \
       (metric in LPIPS_METRICS and getattr(calc, "lpips_scorer", None) is None):
        check_metrics([metric])
    fn = lambda *a: getattr(calc, "calculate_" + base)(*a)
    if part == "":
        return fn(src_image, tgt_image, None, None)
    ms, mt = (1 - src_mask, 1 - tgt_mask) if part == "_unedit_part" else (src_mask, tgt_mask)
    return "nan" if ms.sum() == 0 or mt.sum() == 0 else fn(src_image, tgt_image, ms, mt)


def clip_cells(scorer, metrics, src_image, tgt_image, tgt_mask, src_prompt, tgt_prompt):
    """the CLIP columns of one (image, method) pair in one launch set -> {metric: value or "nan"}"""
    want, imgs, prompts, masks = [], [], [], []
    out = {}
    for m in CLIP_METRICS:
        if m not in metrics:
            continue
        if m == "clip_similarity_target_image_edit_part" and tgt_mask.sum() == 0:
            out[m] = "nan"
            continue
        src = m == "clip_similarity_source_image"
        want.append(m)
        imgs.append(np.asarray(src_image if src else tgt_image).astype(np.uint8))
        prompts.append(src_prompt if src else tgt_prompt)
        masks.append(tgt_mask if m == "clip_similarity_target_image_edit_part" else None)
    if want:
        got = scorer.score(imgs, prompts, masks=masks if any(k is not None for k in masks) else None)
        out.update({m: float(v) for m, v in zip(want, got)})
    return out


def _part_cells(score, names, metrics, src_image, tgt_image, src_mask, tgt_mask):
    """the whole / unedited-part / edited-part columns `names` of one (image, method) pair in one call of score(pred, gt, mask_pred,
    mask_gt) -> {metric: value or "nan"}; the reference's argument order (src_image, tgt_image, ...) and its "nan" rule for empty parts"""
    want, pred, gt, mp, mg = [], [], [], [], []
    out = {}
    for m in names:
        if m not in metrics:
            continue
        part = _split(m)[1]
        ms, mt = (None, None) if part == "" else ((1 - src_mask, 1 - tgt_mask) if part == "_unedit_part" else (src_mask, tgt_mask))
        if part and (ms.sum() == 0 or mt.sum() == 0):
            out[m] = "nan"
            continue
        want.append(m)
        pred.append(src_image); gt.append(tgt_image); mp.append(ms); mg.append(mt)
    if want:
        got = score(pred, gt, mp, mg)
        out.update({m: float(v) for m, v in zip(want, got)})
    return out


def struct_cells(scorer, metrics, src_image, tgt_image, src_mask, tgt_mask):
    """the structure columns of one (image, method) pair in one launch set"""
    return _part_cells(scorer.distance, STRUCT_METRICS, metrics, src_image, tgt_image, src_mask, tgt_mask)


def lpips_cells(scorer, metrics, src_image, tgt_image, src_mask, tgt_mask):
    """the LPIPS columns of one (image, method) pair in one launch set"""
    return _part_cells(scorer.score, LPIPS_METRICS, metrics, src_image, tgt_image, src_mask, tgt_mask)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--annotation_mapping_file", type=str, default="data/mapping_file.json")
    ap.add_argument("--metrics", nargs="+", type=str, default=DEFAULT_METRICS)
    ap.add_argument("--src_image_folder", type=str, default="data/annotation_images")
    ap.add_argument("--tgt_methods", nargs="+", type=str, default=[k for k in all_tgt_image_folders if k.startswith("1_")][:6])
    ap.add_argument("--result_path", type=str, default="evaluation_result.csv")
    ap.add_argument("--device", type=str, default="cuda")
    ap.add_argument("--edit_category_list", nargs="+", type=str, default=[str(i) for i in range(10)])
    ap.add_argument("--evaluate_whole_table", action="store_true")
    # weights of the CLIP columns (not in the reference, which downloads openai/clip-vit-large-patch14)
    ap.add_argument("--checkpoint_dir", type=str, default=None, help="Stable-Diffusion-1.x directory (diffusers layout): text tower + tokenizer")
    ap.add_argument("--clip_model_dir", type=str, default=None, help="local clip-vit-large-patch14 directory: image tower + projections")
    ap.add_argument("--synthetic_weights", action="store_true", help="seeded random towers and the word-level stand-in tokenizer")
    # weights of the structure columns (not in the reference, which downloads facebookresearch/dino:main dino_vitb8)
    ap.add_argument("--dino_checkpoint", type=str, default=None, help="local dino_vitbase8_pretrain.pth: the DINO ViT-B/8 state dict")
    # weights of the LPIPS columns (not in the reference, whose torchmetrics downloads both)
    ap.add_argument("--squeezenet_checkpoint", type=str, default=None, help="local squeezenet1_1-b8a52dc0.pth: torchvision's squeezenet1_1 state dict")
    ap.add_argument("--lpips_checkpoint", type=str, default=None, help="local squeeze.pth of the lpips package: the seven lin layers")
    return ap.parse_args(argv)


def build_scorer(args):
    """ClipScore on a text-only context (no UNet rows, no VAE images) from --checkpoint_dir + --clip_model_dir, or seeded weights"""
    from pnpinversion_amd import checkpoint, weights
    from pnpinversion_amd.clip_score import ClipScore
    from pnpinversion_amd.config import SD1
    from pnpinversion_amd.pipeline import NativePipeline
    if bool(args.synthetic_weights) == bool(args.checkpoint_dir and args.clip_model_dir):
        raise SystemExit("the clip_similarity_* columns need weights: --checkpoint_dir <SD-1.x dir> with --clip_model_dir <clip-vit-large-patch14 dir>, "
                         "or --synthetic_weights (seeded random towers)")
    dev = args.device if args.device != "cuda" else None
    if args.synthetic_weights:
        print(checkpoint.SYNTHETIC_WARNING, file=sys.stderr, flush=True)
        pipe = NativePipeline(SD1, device=dev, max_unet_rows=0, max_vae_images=0, text_encoder="native")
        pipe.engine.load_state_dict(clip_sd=weights.clip_state_dict(SD1, 0))
        scorer = ClipScore(pipe, max_images=3)
        scorer.load_synthetic(0)
        return scorer
    _, _, clip_sd, tok = checkpoint.load_checkpoint_dir(args.checkpoint_dir)
    model_sd = checkpoint.load_clip_model_dir(args.clip_model_dir, text_sd=clip_sd)
    pipe = NativePipeline(SD1, device=dev, max_unet_rows=0, max_vae_images=0, tokenizer=tok, text_encoder="native")
    pipe.engine.load_state_dict(clip_sd=clip_sd)
    scorer = ClipScore(pipe, max_images=3)
    scorer.load_state_dict(model_sd)
    return scorer


def build_struct_scorer(args, engine=None):
    """StructureDistance from --dino_checkpoint, or seeded weights; on the CLIP scorer's context when there is one, else on a context of
    its own (_smallest_engine)"""
    from pnpinversion_amd import checkpoint
    from pnpinversion_amd.structure_distance import StructureDistance
    if args.dino_checkpoint and args.synthetic_weights:
        raise SystemExit("--dino_checkpoint and --synthetic_weights are mutually exclusive")
    scorer = StructureDistance(engine if engine is not None else _smallest_engine(args), max_pairs=3)
    if args.dino_checkpoint:
        scorer.load_state_dict(checkpoint.load_dino_checkpoint(args.dino_checkpoint))
    else:
        print(checkpoint.SYNTHETIC_WARNING, file=sys.stderr, flush=True)
        scorer.load_synthetic(0)
    return scorer


def _smallest_engine(args):
    """a context with no text tower, no UNet rows and no VAE images (the smallest model configuration: its weight arena is never loaded)"""
    import dataclasses
    from pnpinversion_amd.config import TINY16
    from pnpinversion_amd.engine import NativeEngine
    return NativeEngine(dataclasses.replace(TINY16, clip_layers=0), device=args.device if args.device != "cuda" else None,
                        max_unet_rows=0, max_vae_images=0)


def build_lpips_scorer(args, engine=None):
    """Lpips from --squeezenet_checkpoint + --lpips_checkpoint, or seeded weights; on the context that is already there (the CLIP or the
    structure scorer's), else on the smallest one"""
    from pnpinversion_amd import checkpoint
    from pnpinversion_amd.lpips import Lpips
    real = bool(args.squeezenet_checkpoint and args.lpips_checkpoint)
    if real and args.synthetic_weights:
        raise SystemExit("--squeezenet_checkpoint / --lpips_checkpoint and --synthetic_weights are mutually exclusive")
    scorer = Lpips(engine if engine is not None else _smallest_engine(args), max_pairs=3)
    if real:
        scorer.load_state_dict(checkpoint.load_lpips_checkpoint(args.squeezenet_checkpoint, args.lpips_checkpoint))
    else:
        print(checkpoint.SYNTHETIC_WARNING, file=sys.stderr, flush=True)
        scorer.load_synthetic(0)
    return scorer


def run(args, scorer=None, struct_scorer=None, lpips_scorer=None):
    from PIL import Image
    metrics = list(args.metrics)
    check_metrics(metrics, dino=struct_scorer is not None or has_dino_weights(args), lpips=lpips_scorer is not None or has_lpips_weights(args))
    if args.evaluate_whole_table:
        folders = {k: v for k, v in all_tgt_image_folders.items() if k[0] in args.tgt_methods}
    else:
        folders = {k: all_tgt_image_folders[k] for k in args.tgt_methods}
    if scorer is None and any(m in CLIP_METRICS for m in metrics):
        scorer = build_scorer(args)
    if struct_scorer is None and any(m in STRUCT_METRICS for m in metrics):
        struct_scorer = build_struct_scorer(args, engine=getattr(scorer, "engine", None))
    if lpips_scorer is None and any(m in LPIPS_METRICS for m in metrics):
        lpips_scorer = build_lpips_scorer(args, engine=getattr(scorer, "engine", None) or getattr(struct_scorer, "engine", None))
    calc = Calculator(scorer, struct_scorer, lpips_scorer)
    with open(args.result_path, "w", newline="") as f:
        csv.writer(f).writerow(["file_id"] + ["%s|%s" % (k, m) for k in folders for m in metrics])
    with open(args.annotation_mapping_file) as f:
        annotation = json.load(f)
    for key, item in annotation.items():
        if item["editing_type_id"] not in args.edit_category_list:
            continue
        print("evaluating image %s ..." % key)
        mask = mask_decode(item["mask"])[:, :, None].repeat(3, axis=2)
        src_prompt = item["original_prompt"].replace("[", "").replace("]", "")
        tgt_prompt = item["editing_prompt"].replace("[", "").replace("]", "")
        src_image = Image.open(os.path.join(args.src_image_folder, item["image_path"]))
        row = [key]
        for name, folder in folders.items():
            tgt_image = Image.open(os.path.join(folder, item["image_path"]))
            if tgt_image.size[0] != tgt_image.size[1]:            # a multi-panel output: the edit is the right-hand 512 x 512
                w, h = tgt_image.size
                tgt_image = tgt_image.crop((w - 512, h - 512, w, h))
            clip = clip_cells(scorer, metrics, src_image, tgt_image, mask, src_prompt, tgt_prompt) if scorer is not None else {}
            if struct_scorer is not None:
                clip.update(struct_cells(struct_scorer, metrics, src_image, tgt_image, mask, mask))
            if lpips_scorer is not None:
                clip.update(lpips_cells(lpips_scorer, metrics, src_image, tgt_image, mask, mask))
            for m in metrics:
                row.append(clip[m] if m in clip else calculate_metric(calc, m, src_image, tgt_image, mask, mask, src_prompt, tgt_prompt))
        with open(args.result_path, "a+", newline="") as f:
            csv.writer(f).writerow(row)


if __name__ == "__main__":
    _args = parse_args()
    check_metrics(_args.metrics, dino=has_dino_weights(_args), lpips=has_lpips_weights(_args))
    run(_args)
