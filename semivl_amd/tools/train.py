"""`python -m semivl_amd.tools.train --config cfg.yaml --save-path DIR [--resume [FILE]] [--labeled-id-path F]
[--unlabeled-id-path F]`

The training script of the reference (semivl.py:60-433; third_party/unimatch/supervised.py for cfg['method'] =
'supervised') on the native path: `semivl_amd.trainer.train` with the config read from yaml.  DIR receives config.yaml,
train.log, metrics.jsonl, latest.pth, best.pth and debug/*.png.  `--resume` without a file continues DIR/latest.pth.  The
id paths default to the reference's splits/<dataset>/<split>/{labeled,unlabeled}.txt.  Under
`python -m torch.distributed.run` it initialises the process group from the environment, like tools/eval.py; otherwise it
runs single-process."""
import argparse
import os

import torch
import torch.distributed as dist


def _parser():
    ap = argparse.ArgumentParser(description="Train a SemiVL (or supervised) model: epochs, evaluation, checkpoints, resume")
    ap.add_argument("--config", required=True, help="yaml config of the run")
    ap.add_argument("--save-path", required=True, help="directory for checkpoints, logs, metrics and debug panels")
    ap.add_argument("--resume", nargs="?", const="", default=None, metavar="FILE",
                    help="continue from FILE (default: SAVE_PATH/latest.pth)")
    ap.add_argument("--labeled-id-path", default=None, help="split file of the labelled ids")
    ap.add_argument("--unlabeled-id-path", default=None, help="split file of the unlabelled ids")
    return ap


def main(argv=None):
    """Returns what `trainer.train` returns."""
    import yaml
    from ..trainer import default_id_paths, train
    args = _parser().parse_args(argv)
    with open(args.config) as f:
        cfg = yaml.load(f, Loader=yaml.Loader)
    cfg.setdefault("text_embedding_variant", None)          # legacy config support, as tools/eval.py
    cfg.setdefault("pl_text", cfg["text_embedding_variant"])
    labeled, unlabeled = args.labeled_id_path, args.unlabeled_id_path
    if labeled is None or unlabeled is None:
        dl, du = default_id_paths(cfg)
        labeled, unlabeled = labeled or dl, unlabeled or du
    resume = args.resume
    if resume == "":
        resume = os.path.join(args.save_path, "latest.pth")
    local_rank, own_group = 0, False
    if "RANK" in os.environ and "WORLD_SIZE" in os.environ:          # launched by torch.distributed.run
        local_rank = int(os.environ.get("LOCAL_RANK", 0))
        torch.cuda.set_device(local_rank)
        if not dist.is_initialized():
            dist.init_process_group("nccl")
            own_group = True
    try:
        return train(cfg, args.save_path, labeled, unlabeled, resume=resume, device=torch.device("cuda", local_rank))
    finally:
        if own_group:
            dist.destroy_process_group()


if __name__ == "__main__":
    main()
