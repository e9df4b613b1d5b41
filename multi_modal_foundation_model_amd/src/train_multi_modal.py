"""Entry script: masked pretraining of the spike + behaviour MultiModal model on an MI355X.

Same flags, config files, model/optimiser/scheduler/trainer construction order as the reference's
`src/train_multi_modal.py`; the session data comes from the synthetic loader because the HuggingFace
datasets (`neurofm123/<eid>_aligned`, reference lines 97-119) cannot be downloaded offline.  Any
iterable yielding the loader batch dict (loader/base.py:436-450) can be passed instead.

    cd multi_modal_foundation_model_amd && python src/train_multi_modal.py --mixed_training --epochs 2
    torchrun --nproc-per-node 8 --master-addr 127.0.0.1 src/train_multi_modal.py --mixed_training
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(os.path.dirname(HERE))):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch
from torch.optim.lr_scheduler import OneCycleLR

from multi_modal.decoder_embeddings import DecoderEmbedding
from multi_modal.encoder_embeddings import EncoderEmbedding
from multi_modal.mm import MultiModal
from multi_modal_foundation_model_amd.ddp import Accelerator
from multi_modal_foundation_model_amd.optim import freeze_parameters, make_optimizer
from multi_modal_foundation_model_amd.synthetic import MultiSessionLoader, SyntheticLoader
from trainer.base import accumulation_groups, validate_accumulation_steps
from trainer.make import make_multimodal_trainer
from utils.config_utils import config_from_kwargs, update_config
from utils.utils import set_seed

AVAIL_MOD = ["ap", "behavior"]


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--eid", type=str, default="synthetic-session")
    ap.add_argument("--mask_ratio", type=float, default=0.1)
    ap.add_argument("--mask_mode", type=str, default="temporal")
    ap.add_argument("--use_MtM", action="store_true")
    ap.add_argument("--mixed_training", action="store_true")
    ap.add_argument("--overwrite", action="store_true")
    ap.add_argument("--base_path", type=str, default="/tmp/mmfm_results")
    ap.add_argument("--epochs", type=int, default=None, help="override training.num_epochs (2000 upstream)")
    ap.add_argument("--grad_accum_steps", type=int, default=None,
                    help="override optimizer.gradient_accumulation_steps: batches per optimiser step (the mean gradient of the group is applied)")
    ap.add_argument("--batches_per_epoch", type=int, default=8)
    ap.add_argument("--n_neurons", type=int, default=668)
    ap.add_argument("--dtype", type=str, default=os.environ.get("MMFM_DTYPE", "fp32"), choices=["fp32", "bf16"])
    # the reference edits `modal_filter` in the script: spikes -> behaviour (decoding), behaviour -> spikes (encoding) and the single-modality
    # baselines are `--modal_filter_input ap --modal_filter_output behavior` and so on.  The two lists need equally many modalities
    ap.add_argument("--modal_filter_input", type=str, nargs="+", default=list(AVAIL_MOD), choices=AVAIL_MOD,
                    help="modalities the encoder gets tokenisers for")
    ap.add_argument("--modal_filter_output", type=str, nargs="+", default=list(AVAIL_MOD), choices=AVAIL_MOD,
                    help="modalities the decoder gets tokenisers and heads for")
    # fine-tuning on a frozen trunk: fnmatch patterns over parameter names (`encoder.*`, `*_embeddings.*.embedder.*`, ...).  The named
    # parameters get requires_grad = False before the optimiser is made; the engine then launches only the backward the others need
    ap.add_argument("--freeze", type=str, nargs="*", default=None,
                    help="fnmatch patterns of parameter names to freeze (overrides training.freeze of the trainer config)")
    ap.add_argument("--input_masking", action="store_true",
                    help="train with mask_type: input (training.mask_mode sampled per step; per-element corruption and loss masks) "
                         "instead of failing on it as upstream does: sets training.mask_type = input and training.input_masking")
    ap.add_argument("--neuron_padding", action="store_true",
                    help="honour the loader's space_attn_mask: padded spike channels are zeroed on both sides and leave the loss and "
                         "n_examples (sets training.neuron_padding)")
    ap.add_argument("--context_mask", action="store_true",
                    help="honour context.forward / context.backward of the model config: the encoder's self-attention and the "
                         "cross-attention see a key only inside that window over the time stamps (sets training.context_mask)")
    ap.add_argument("--per_sample_mask", action="store_true",
                    help="zero each sample's tokens where its own mask is 1 instead of where the first sample's is, on both sides (sets "
                         "training.per_sample_mask)")
    ap.add_argument("--n_sessions", type=int, default=1,
                    help="K > 1: multi-session pretraining on synthetic sessions of 300..n_neurons neurons each, batch i from session "
                         "i %% K, spikes right-padded with -1 up to n_neurons (1: one session, no padding)")
    ap.add_argument("--use_session", action="store_true",
                    help="per-session read-in / read-out layers (sets model.use_session): every session's n_k neurons are mapped to a shared "
                         "width in front of the spike tokenisers and back behind the head; with --n_sessions K the sizes are the loader's, "
                         "a single session trains as {eid: n_neurons}")
    ap.add_argument("--stitch_width", type=int, default=None, help="the shared width P of --use_session (model.stitcher.width; default n_neurons)")
    return ap


def modal_filter_of(args):
    """The reference's `modal_filter` dict from the two flags, each list in avail_mod order (the construction order of the tokenisers)."""
    return {"input": [m for m in AVAIL_MOD if m in args.modal_filter_input], "output": [m for m in AVAIL_MOD if m in args.modal_filter_output]}


def main(argv=None):
    args = build_parser().parse_args(argv)
    os.chdir(os.path.dirname(HERE))           # config paths are 'src/configs/...' like upstream

    avail_beh = ["wheel-speed", "whisker-motion-energy"]
    config = config_from_kwargs({"model": "include:src/configs/multi_modal/mm.yaml"})
    config = update_config("src/configs/multi_modal/trainer_mm.yaml", config)
    config["model"]["masker"]["mode"] = args.mask_mode
    config["model"]["masker"]["ratio"] = args.mask_ratio
    if args.epochs is not None:
        config["training"]["num_epochs"] = args.epochs
    if args.grad_accum_steps is not None:
        config["optimizer"]["gradient_accumulation_steps"] = args.grad_accum_steps
    if args.input_masking:
        config["training"]["mask_type"] = "input"
        config["training"]["input_masking"] = True
    if args.neuron_padding:
        config["training"]["neuron_padding"] = True
    if args.context_mask:
        config["training"]["context_mask"] = True
    if args.per_sample_mask:
        config["training"]["per_sample_mask"] = True
    if args.n_sessions < 1:
        raise ValueError(f"--n_sessions must be >= 1, got {args.n_sessions}")
    if args.stitch_width is not None and not args.use_session:
        raise ValueError("--stitch_width belongs to --use_session")
    if args.use_session:
        config["model"]["use_session"] = True
        config["model"]["stitcher"] = dict(config["model"].get("stitcher") or {}, width=args.stitch_width if args.stitch_width is not None else args.n_neurons)
    set_seed(config.seed)

    avail_mod = list(AVAIL_MOD)
    modal_filter = modal_filter_of(args)
    mask_mode = "-".join(config.training.mask_mode) if config.training.mask_type == "input" else args.mask_mode
    log_dir = os.path.join(args.base_path, "results", f"ses-{args.eid}", "set-train", f"inModal-{'-'.join(modal_filter['input'])}",
                           f"outModal-{'-'.join(modal_filter['output'])}", f"mask-{config.training.mask_type}", f"mode-{mask_mode}",
                           f"ratio-{args.mask_ratio}", f"mixedTraining-{args.mixed_training}")
    assert not os.path.exists(os.path.join(log_dir, "model_last.pt")) or args.overwrite, "last checkpoint exists and overwrite is False"
    os.makedirs(log_dir, exist_ok=True)

    accelerator = Accelerator()
    n_behaviors, n_neurons = len(avail_beh), args.n_neurons
    meta_data = {"num_neurons": [n_neurons], "eids": [args.eid]}
    T = config.data.max_time_length
    if args.n_sessions > 1:
        train_dataloader = MultiSessionLoader(args.batches_per_epoch, config.training.train_batch_size, T, n_neurons, n_behaviors,
                                              n_sessions=args.n_sessions, rank=accelerator.rank, seed0=0, world=accelerator.world)
        val_dataloader = MultiSessionLoader(2, config.training.test_batch_size, T, n_neurons, n_behaviors, n_sessions=args.n_sessions,
                                            rank=accelerator.rank, seed0=10 ** 6, world=accelerator.world)
    else:
        train_dataloader = SyntheticLoader(args.batches_per_epoch, config.training.train_batch_size, T, n_neurons, n_behaviors,
                                           rank=accelerator.rank, seed0=0)
        val_dataloader = SyntheticLoader(2, config.training.test_batch_size, T, n_neurons, n_behaviors, rank=accelerator.rank, seed0=10 ** 6)

    # --use_session: the spike tokenisers and the head run at the shared width; the sessions are the loader's (eid session{k}, its
    # sizes) or the one session this run trains
    n_ap = config["model"]["stitcher"]["width"] if args.use_session else n_neurons
    if args.use_session:
        sizes = train_dataloader.sizes if args.n_sessions > 1 else None
        meta_data["sessions"] = {f"session{k}": n for k, n in enumerate(sizes)} if sizes else {"synthetic": n_neurons}
    encoder_embeddings, decoder_embeddings = {}, {}
    for mod in modal_filter["input"]:
        encoder_embeddings[mod] = EncoderEmbedding(hidden_size=config.model.encoder.transformer.hidden_size,
                                                   n_channel=n_ap if mod == "ap" else n_behaviors, config=config.model.encoder)
    for mod in modal_filter["output"]:
        decoder_embeddings[mod] = DecoderEmbedding(hidden_size=config.model.decoder.transformer.hidden_size,
                                                   n_channel=n_ap if mod == "ap" else n_behaviors,
                                                   output_channel=n_ap if mod == "ap" else n_behaviors, config=config.model.decoder)

    model = MultiModal(encoder_embeddings, decoder_embeddings, avail_mod=avail_mod, config=config.model,
                       share_modality_embeddings=True, **config.method.model_kwargs, **meta_data)
    model.compute_dtype = args.dtype
    print("(train) masking mode: ", model.masker.mode)
    print("(train) masking ratio: ", model.masker.ratio)
    print("(train) masking active: ", model.masker.force_active)
    model = accelerator.prepare(model)

    # training.freeze is no key of the reference's YAML either: absent or empty freezes nothing
    frozen = freeze_parameters(model, args.freeze if args.freeze is not None else config.training.get("freeze", None))
    if frozen:
        print(f"(train) frozen: {len(frozen)} parameter tensors ({frozen[0]} .. {frozen[-1]})")

    # optimizer.max_grad_norm is no key of the reference's YAML: absent or null builds the reference's optimiser (one launch per step),
    # a number turns on the fused clip (optim.py)
    optimizer = make_optimizer(model, lr=config.optimizer.lr, weight_decay=config.optimizer.wd, eps=config.optimizer.eps,
                               max_grad_norm=config.optimizer.get("max_grad_norm", None))
    # one scheduler step per optimiser step, one optimiser step per group of gradient_accumulation_steps batches; the last group of an
    # epoch closes short (trainer/base.py, accumulation_groups).  Upstream's floor(epochs * batches / k) is this number for k = 1 and
    # whenever k divides the epoch length - the only cases in which OneCycleLR ends on the last optimiser step with it
    k = validate_accumulation_steps(config.optimizer.gradient_accumulation_steps)
    lr_scheduler = OneCycleLR(optimizer=optimizer,
                              total_steps=config.training.num_epochs * len(accumulation_groups(len(train_dataloader), k)),
                              max_lr=config.optimizer.lr, pct_start=config.optimizer.warmup_pct, div_factor=config.optimizer.div_factor)

    trainer_ = make_multimodal_trainer(model=model, train_dataloader=train_dataloader, eval_dataloader=val_dataloader,
                                       optimizer=optimizer, log_dir=log_dir, accelerator=accelerator, lr_scheduler=lr_scheduler,
                                       avail_mod=avail_mod, modal_filter=modal_filter, mixed_training=args.mixed_training, config=config,
                                       **meta_data)
    trainer_.train()


if __name__ == "__main__":
    main()
