#!/usr/bin/env python
"""PIE-Bench sweep driver with the CLI of the reference's run_editing_p2p.py (same flags, same output tree, same
skip-if-exists resume), on the MI355X-native P2PEditor.  Under torch.distributed.run (one process per GPU) the ordered work
list is sharded round-robin over the ranks and the weight arena is broadcast once from rank 0 over RCCL / xGMI; there is no
per-image communication (pnpinversion_amd/sweep.py)."""
import argparse

from pnpinversion_amd import sweep
from pnpinversion_amd.p2p_editor import P2PEditor
from pnpinversion_amd.sweep import mask_decode, setup_seed  # noqa: F401  (the reference script's surface: tests and tools import them from here)

BATCHED_METHODS = ("directinversion+p2p",)     # methods with a several-images-per-launch entry point (always the lock-step schedule)
EDIT_KW = dict(guidance_scale=7.5, cross_replace_steps=0.4, self_replace_steps=0.6)
PROXIMAL_KW = dict(proximal="l0", quantile=0.75, use_inversion_guidance=True, recon_lr=1, recon_t=400)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    sweep.add_sweep_args(ap, ["directinversion+p2p"])
    ap.add_argument("--batch_size", type=int, default=1, help="images per set of launches and GPU (not in the reference: it edits one by one)")
    ap.add_argument("--overlap_stages", dest="overlap_stages", action="store_true", default=True,
                    help="directinversion+p2p, batch_size 1 (default): invert the next image on a second HIP stream while this one is "
                         "edited -- same panels, about 12 %% more images per second")
    ap.add_argument("--no_overlap_stages", dest="overlap_stages", action="store_false", help="edit strictly one image after the other")
    ap.add_argument("--images_in_flight", type=int, default=3,
                    help="batch_size 1 (default 3; not in the reference, which edits one by one): image i is edited on library context "
                         "i %% N of this GPU, each context with its own HIP stream and worker thread -- the one-row launch chains of an edit "
                         "leave most of the chip idle between dependent launches, independent chains fill the gaps; same panels.  "
                         "Measured on MI355X: directinversion+p2p 0.90 -> 1.11 images/s at 3, null-text-inversion+p2p 2.1x at 4.  "
                         "1 = one image after the other (then --overlap_stages applies)")
    ap.add_argument("--num_ddim_steps", type=int, default=50)
    return ap.parse_args(argv)


def blend_args(blended_word):
    """the mapping file's `blended_word` ("cat dog" or "") -> (blend_word, eq_params) of the editor, (None, None) without one"""
    if blended_word == "":
        return None, None
    blended = blended_word.split(" ")
    return ((blended[0],), (blended[1],)), {"words": (blended[1],), "values": (2,)}


def main(argv=None):
    args = parse_args(argv)
    from pnpinversion_amd.config import SD1, SMALL64
    from pnpinversion_amd.pipeline import NativePipeline
    batched = args.batch_size > 1 and any(m in BATCHED_METHODS for m in args.edit_method_list)
    if args.batch_size > 1:
        for m in args.edit_method_list:
            if m not in BATCHED_METHODS:
                print(f"WARNING: --batch_size {args.batch_size} applies to {BATCHED_METHODS} only; [{m}] is edited one image at a time")
    make_pipeline = lambda cfg, device, tokenizer: NativePipeline(                                      # noqa: E731
        cfg, device=device, max_unet_rows=12 * (args.batch_size if batched else 1), text_encoder="native", tokenizer=tokenizer)
    with sweep.session(args, {"sd1": SD1, "small64": SMALL64}, make_pipeline) as s:
        editor = P2PEditor(args.edit_method_list, s.device, num_ddim_steps=args.num_ddim_steps, pipeline=s.pipe)
        instructions = sweep.read_mapping(args)
        for method in args.edit_method_list:
            todo = [(image_path, sweep.clean_prompt(item["original_prompt"]), sweep.clean_prompt(item["editing_prompt"]),
                     *blend_args(item["blended_word"]), out_path)
                    for item, image_path, out_path in sweep.plan(args, instructions, method, s.rank, s.world)]
            nb = args.batch_size if method in BATCHED_METHODS else 1
            stream = None                      # image after image through one call: (image_path, src, tgt, blend_word, eq_params) each
            if args.images_in_flight > 1 and nb == 1 and len(todo) >= 2:      # nothing / one image to edit: no extra contexts
                setup_seed()
                stream = editor.edit_stream_in_flight(method, [c[:5] for c in todo], n_flight=args.images_in_flight, **EDIT_KW, **PROXIMAL_KW)
            elif args.overlap_stages and nb == 1 and method == "directinversion+p2p":
                setup_seed()
                stream = editor.edit_stream_directinversion([c[:5] for c in todo], **EDIT_KW)
            if stream is not None:
                for c, panel in zip(todo, stream):
                    print(f"editing image [{c[0]}] with [{method}]")
                    sweep.save_panel(panel, c[5])
                continue
            for b0 in range(0, len(todo), nb):
                chunk = todo[b0:b0 + nb]
                for c in chunk:
                    print(f"editing image [{c[0]}] with [{method}]")
                setup_seed()
                if len(chunk) == 1:
                    image_path, src, tgt, blend_word, eq_params, _ = chunk[0]
                    panels = [editor(method, image_path=image_path, prompt_src=src, prompt_tar=tgt, blend_word=blend_word, eq_params=eq_params,
                                     **EDIT_KW, **PROXIMAL_KW)]
                else:   # several images per set of launches (12 UNet rows each); same per-image schedule and results
                    panels = editor.edit_images_directinversion([c[0] for c in chunk], [c[1] for c in chunk], [c[2] for c in chunk], **EDIT_KW,
                                                                blend_words=[c[3] for c in chunk], eq_params=[c[4] for c in chunk])
                for panel, c in zip(panels, chunk):
                    sweep.save_panel(panel, c[5])
        if hasattr(editor, "close_peers"):
            editor.close_peers()             # the extra library contexts of the in-flight sweep


if __name__ == "__main__":
    main()
