"""Train from a dataset directory (the reference's open_loop_training/train.py with configs/thinktwice.py):

    python -m thinktwice_amd.train --data-root <dir the route paths are relative to> --metadata <dataset_metadata.pkl> \\
        --work-dir work --epochs 60 --batch-size 8 [--cumulative-iters 2] [--resume auto] [--load-from weights.pth] \\
        [--metrics] [--save-best wp_ade_5 | --save-best seg_miou:greater]
    python -m torch.distributed.run --nproc_per_node 8 -m thinktwice_amd.train ...          # one rank per GPU

It builds the model, a trainer.Trainer, the train and validation dataset.DatasetIndex and loader.DeviceBatchLoader and hands
them to runner.EpochRunner.  The towns, caps and label classes are the reference's (data_config.py); `--dev` is its is_dev
branch.  Under torch.distributed.run rank and world come from the environment."""
import argparse
import datetime
import os

DTYPES = ("f32", "f32x3")


def parse_args(argv=None):
    from . import data_config as dc
    ap = argparse.ArgumentParser(prog="python -m thinktwice_amd.train", description=__doc__.split("\n\n")[0])
    ap.add_argument("--data-root", required=True, help="the directory the dataset's route paths are relative to (the reference's "
                    "working directory: routes are ../dataset/<town>/<route> from it)")
    ap.add_argument("--metadata", default=None, help="dataset_metadata.pkl (default: <data-root>/../dataset/dataset_metadata.pkl)")
    ap.add_argument("--work-dir", required=True, help="checkpoints and log.json go here")
    ap.add_argument("--epochs", type=int, default=dc.TOTAL_EPOCHS)
    ap.add_argument("--batch-size", type=int, default=dc.BATCH_SIZE_PER_GPU, help="per GPU")
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--cumulative-iters", type=int, default=1, metavar="K", help="accumulate gradients over K iterations per "
                    "optimizer update (mmcv GradientCumulativeOptimizerHook): the effective global batch is world x batch-size x K; "
                    "the reference's recipe, lr 1e-4, is a global batch of 128")
    ap.add_argument("--dtype", choices=DTYPES, default="f32x3", help="convolution arithmetic: exact f32 or the bf16x3 split")
    ap.add_argument("--final-dim", type=int, nargs=2, default=None, metavar=("H", "W"), help="reduced image size (default 448 896)")
    ap.add_argument("--dev", action="store_true", help="the reference's is_dev split: town01_00, 10 samples")
    ap.add_argument("--frozen-bn", action="store_true", help="BatchNorm on its running statistics (fine-tuning)")
    ap.add_argument("--no-augment", action="store_true", help="no colour augmentation of the training frames")
    ap.add_argument("--resume", default=None, metavar="auto|FILE", help="continue from <work-dir>/latest.pth or a checkpoint file")
    ap.add_argument("--log-interval", type=int, default=100)
    ap.add_argument("--load-from", default=None, help="initial weights (a checkpoint or a bare state_dict); default: init_params")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--train-towns", nargs="+", default=None, help="override the split's training towns")
    ap.add_argument("--val-towns", nargs="+", default=None, help="override the split's validation towns")
    ap.add_argument("--metrics", action="store_true", help="the validation pass also reports the open-loop task metrics "
                    "(evaluate.MetricWindow: waypoint errors in metres, seg IoU, depth-bin accuracy), from the same forwards")
    ap.add_argument("--save-best", default=None, metavar="NAME[:greater]", help="keep the checkpoint with the best validation "
                    "value of a logged name as best_NAME.pth: the lowest, or with :greater the highest (seg_miou)")
    args = ap.parse_args(argv)
    if args.save_best is not None:
        from .runner import parse_save_best
        try:
            parse_save_best(args.save_best)
        except ValueError as e:
            ap.error(str(e))
    return args


def assemble(args):
    """Everything main() needs that is not on the device: the dataset cfg, the augmentation conf, the model overrides and the
    runner's arguments, from the parsed arguments."""
    from . import data_config as dc
    cfg = dc.data_config(dev=args.dev)
    if args.train_towns:
        cfg["train_town"] = list(args.train_towns)
    if args.val_towns:
        cfg["val_town"] = list(args.val_towns)
    final_dim = tuple(args.final_dim) if args.final_dim else None
    metadata = args.metadata or os.path.join(args.data_root, "..", "dataset", "dataset_metadata.pkl")
    runner_extra = {}
    if getattr(args, "metrics", False):
        runner_extra["metrics"] = True
    if getattr(args, "save_best", None):
        from .runner import parse_save_best
        runner_extra["save_best"], runner_extra["save_best_rule"] = parse_save_best(args.save_best)
    return {"cfg": cfg, "ida_aug_conf": dc.ida_aug_conf(final_dim), "overrides": {} if final_dim is None else {"final_dim": final_dim},
            "metadata": metadata, "root": args.data_root, "cumulative_iters": args.cumulative_iters,
            "trainer": dict(lr=args.lr, frozen_bn=bool(args.frozen_bn)),
            "loader": dict(batch_size=args.batch_size, seed=args.seed, augment=not args.no_augment),
            "runner": dict(work_dir=args.work_dir, max_epochs=args.epochs, log_interval=args.log_interval,
                           ckpt_interval=dc.CKPT_INTERVAL, eval_interval=dc.EVAL_INTERVAL, **runner_extra)}


def main(argv=None):
    args = parse_args(argv)
    conf = assemble(args)
    import torch
    import torch.distributed as dist
    from . import dataset, model as tm, params
    from .loader import DeviceBatchLoader
    from .runner import EpochRunner
    from .trainer import Trainer
    if not torch.cuda.is_available():
        raise SystemExit("thinktwice_amd.train needs a GPU: there is no CPU path")
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    started = False
    if world > 1 and not dist.is_initialized():
        dist.init_process_group(backend="nccl", device_id=device, timeout=datetime.timedelta(minutes=4))
        started = True
    try:
        dtype = torch.float32 if args.dtype == "f32" else "f32x3"
        model, mcfg = tm.build_thinktwice(dtype=dtype, device=device, **conf["overrides"])
        if args.load_from:
            sd = torch.load(args.load_from, map_location="cpu", weights_only=False)
            sd = sd.get("state_dict", sd)
        else:
            sd = params.init_params(mcfg, seed=args.seed)
        trainer = Trainer(model, sd, **conf["trainer"])
        cfg = conf["cfg"]
        train_index = dataset.DatasetIndex(conf["metadata"], cfg["train_town"], cfg, root=conf["root"])
        train_loader = DeviceBatchLoader(train_index, cfg, conf["ida_aug_conf"], device=device, train=True, rank=rank, world=world,
                                         **conf["loader"])
        val_loader = None
        val_index = dataset.DatasetIndex(conf["metadata"], cfg["val_town"], cfg, root=conf["root"])
        if len(val_index):
            val_loader = DeviceBatchLoader(val_index, cfg, conf["ida_aug_conf"], device=device, train=False, rank=rank, world=world,
                                           batch_size=args.batch_size, seed=args.seed)
        runner = EpochRunner(trainer, train_loader, val_loader, verbose=rank == 0, cumulative_iters=conf["cumulative_iters"],
                             **conf["runner"])
        if rank == 0:
            print(f"effective global batch: {world} x {args.batch_size} x {conf['cumulative_iters']} = "
                  f"{world * args.batch_size * conf['cumulative_iters']} (world x batch-size x cumulative-iters)", flush=True)
        try:
            if args.resume:
                runner.resume(args.resume)
            return runner.run()
        finally:
            train_loader.close()
            if val_loader is not None:
                val_loader.close()
    finally:
        if started:
            dist.destroy_process_group()


if __name__ == "__main__":
    main()
