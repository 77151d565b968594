"""`python -m semivl_amd.tools.eval --config cfg.yaml --save-path ckpt.pth [--ema] [--pred-path DIR] [--logit-path DIR]
[--eval-mode MODE] [--report-json FILE]`

The stand-alone evaluator of the reference (third_party/unimatch/eval.py:85-162) on the native path: the validation split
through data.ValLoader, `report.evaluate_report` (confusion table counted on the device, cfg['eval_tta'] /
cfg['eval_report'] from the config), the metric table and the mIoU line printed by rank 0.  Like the reference it builds the
model without the guidance encoder (cfg['clip_encoder'] = None), loads `--save-path` with the rules of `load_checkpoint`
('none': no checkpoint) and defaults the mode to 'sliding_window' for Cityscapes and 'original' otherwise.  Under
`python -m torch.distributed.run` it initialises the process group from the environment and shards the split over the
ranks; otherwise it runs single-process."""
import argparse
import json
import os

import torch
import torch.distributed as dist


def _parser():
    ap = argparse.ArgumentParser(description="Evaluate a checkpoint: metric table, confusion matrix, palette PNGs, logits")
    ap.add_argument("--config", required=True, help="yaml config of the run")
    ap.add_argument("--save-path", required=True, help="checkpoint file, or 'none'")
    ap.add_argument("--ema", action="store_true", help="evaluate the checkpoint's 'ema_model' entry")
    ap.add_argument("--pred-path", default=None, help="directory for the predictions as palette PNGs")
    ap.add_argument("--logit-path", default=None, help="directory for the class scores as .pt files")
    ap.add_argument("--eval-mode", default=None, help="overrides cfg['eval_mode']")
    ap.add_argument("--report-json", default=None, help="file for EvalReport.to_dict() as JSON (rank 0)")
    return ap


def main(argv=None):
    """Returns the EvalReport (every rank holds the all-reduced table)."""
    import yaml
    from ..checkpoint import load_checkpoint
    from ..data import GpuAugmenter, ValLoader
    from ..model.builder import build_model
    from ..report import evaluate_report
    args = _parser().parse_args(argv)
    with open(args.config) as f:
        cfg = yaml.load(f, Loader=yaml.Loader)
    cfg.setdefault("text_embedding_variant", None)          # legacy config support (eval.py:91-93)
    cfg.setdefault("pl_text", cfg["text_embedding_variant"])
    cfg["clip_encoder"] = None
    rank, world, local_rank, own_group = 0, 1, 0, False
    if "RANK" in os.environ and "WORLD_SIZE" in os.environ:          # launched by torch.distributed.run
        local_rank = int(os.environ.get("LOCAL_RANK", 0))
        torch.cuda.set_device(local_rank)
        if not dist.is_initialized():
            dist.init_process_group("nccl")
            own_group = True
        rank, world = dist.get_rank(), dist.get_world_size()
    device = torch.device("cuda", local_rank)
    try:
        model = build_model(cfg)
        model.to(device)
        if args.save_path != "none":
            epoch = load_checkpoint(args.save_path, model, ema=args.ema)
            if rank == 0:
                print("************ Load from checkpoint at epoch %i\n" % epoch)
        elif rank == 0:
            print("************ WARNING: NO CHECKPOINT SPECIFIED")
        mode = args.eval_mode or cfg.get("eval_mode") or ("sliding_window" if cfg["dataset"] == "cityscapes" else "original")
        loader = ValLoader(cfg, GpuAugmenter.from_cfg(cfg, device=device), rank, world)
        with torch.cuda.device(device):
            rep = evaluate_report(model, loader, mode, cfg, pred_path=args.pred_path, logit_path=args.logit_path)
        if rank == 0:
            print(rep.format_table())
            print("***** Evaluation {} ***** >>>> MeanIoU: {:.2f}\n".format(mode, rep.miou))
            if args.report_json is not None:
                os.makedirs(os.path.dirname(os.path.abspath(args.report_json)), exist_ok=True)
                with open(args.report_json, "w") as f:
                    json.dump(dict(rep.to_dict(), eval_mode=mode, images=len(loader.set), world=world), f)
    finally:
        if own_group:
            dist.destroy_process_group()
    return rep


if __name__ == "__main__":
    main()
