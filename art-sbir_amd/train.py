"""Drop-in for /root/reference/train.py on MI355X (same CLI flags, same outputs).

  get_loss        train.py:27-37  three separate encoder forwards (-> per-branch
                                  BatchNorm statistics), dispatch on the output arity
  triplet_train   train.py:39-98  epochs / iteration-level losses / timing dict
  CLI             train.py:103-195
Differences, all opt-in or documented:
  * the model, loss and optimizer run on libartsbir_hip (models.ModifiedResNet,
    losses.*, optim.Adam); ``--dtype bf16`` selects the MFMA bf16 throughput mode
    (default f32 = the reference's arithmetic);
  * get_loss dispatches on the output TYPE, not ``len(output) > 3`` (the
    reference misfires for a plain model at batch size <= 3);
  * the reference evaluates its test loss on the stale last TRAIN batch
    (train.py:80,89); that is reproduced by default (drop-in), ``--fresh_eval``
    evaluates on the test batches instead;
  * data: the Sketchy/Kaggle files are not available offline — ``-d Synthetic``
    (default) generates the triplets (data_preparation.SyntheticTripletDataset);
  * one process per GPU when launched by torch.distributed.run: minibatches
    are sharded and gradients all-reduced over RCCL (ddp.py);
  * ``--negatives hardest|semihard`` replaces the negative the dataset drew by
    one mined among the 2 x batch gallery-side embeddings of the step
    (losses.MinedNegatives); every process mines in its own shard;
  * ``--memory_size M`` adds a ring of the last M gallery-side embeddings to the
    candidates of ``--negatives`` (losses.CrossBatchMemory); under
    torch.distributed.run the ring holds every rank's rows, so negatives cross ranks;
  * ``--negatives all --loss_type cosine`` trains with the InfoNCE (softmax contrastive)
    loss over all 2 x batch gallery-side embeddings of the step and the ring
    (losses.InfoNCELoss), at ``--temperature``;
  * ``--gather_negatives`` (with ``--negatives all``, under torch.distributed.run) makes the
    gallery-side embeddings of every rank the candidates of that loss: one all-gather in the
    forward, the gathered rows' gradients summed and sent home in the backward.
"""
from __future__ import annotations

import argparse
import os
from timeit import default_timer as timer

import torch
from torch.utils.data import DataLoader

import data_preparation
import ddp
import inference
import losses
import models
import optim
import utils
import visualization

device = "cuda" if torch.cuda.is_available() else "cpu"


def get_loss(loss_fn, model, elements):
    if isinstance(loss_fn, (losses.MinedNegatives, losses.InfoNCELoss)):
        # the items end with the positive's and the negative's photo number
        # (get_datasets(ids=True)): the identities of the 2B mining candidates
        cand_ids = torch.cat((elements[-2], elements[-1]))
        return _get_loss(lambda *a: loss_fn(*a, cand_ids=cand_ids), model, elements[:-2])
    return _get_loss(loss_fn, model, elements)


def _get_loss(loss_fn, model, elements):
    # three forward calls (per-branch BatchNorm statistics, train.py:28-30), run
    # as one batched encoder pass when the model offers it
    if hasattr(model, "forward_branches") and elements[0].shape == elements[1].shape == elements[2].shape:
        s, p, n = model.forward_branches(elements[:3])
    else:
        s = model(elements[0])
        p = model(elements[1])
        n = model(elements[2])
    if isinstance(s, torch.Tensor):
        return loss_fn(s, p, n)
    if len(s) == 2:
        return loss_fn(s[0], p[0], n[0], s[1], p[1], elements[3])
    return loss_fn(s[0], p[0], n[0], s[1], p[1], s[2], p[2], elements[3], elements[4])


def triplet_train(model, epochs, train_dataloader, test_dataloader, loss_fn, optimizer, with_classification,
                  stale_eval=True):
    # the training loop runs on a high-priority stream, so the dispatcher serves
    # the data-gradient / BatchNorm chain ahead of the weight gradients that the
    # engine overlaps on its side stream
    if torch.device(device).type == "cuda":
        with torch.cuda.stream(torch.cuda.Stream(device=device, priority=-1)):
            return _triplet_train(model, epochs, train_dataloader, test_dataloader, loss_fn, optimizer,
                                  with_classification, stale_eval)
    return _triplet_train(model, epochs, train_dataloader, test_dataloader, loss_fn, optimizer, with_classification,
                          stale_eval)


def _triplet_train(model, epochs, train_dataloader, test_dataloader, loss_fn, optimizer, with_classification,
                   stale_eval=True):
    start_time = timer()
    reducer = ddp.attach_overlapped_reducer(model)
    train_losses, test_losses, itrain_losses, itest_losses = [], [], [], []
    mining = isinstance(loss_fn, losses.MinedNegatives)
    mined_fraction = []  # per epoch: the share of training anchors whose negative was replaced
    with_memory = mining and loss_fn.memory is not None
    memory_fraction = []  # per epoch: the share whose negative came from the cross-batch memory
    contrastive = isinstance(loss_fn, losses.InfoNCELoss)
    positive_probability = []  # per epoch: the mean softmax probability of the positive (InfoNCE)
    iteration_loss_frequency = 10000 // train_dataloader.batch_size if epochs <= 6 else 0
    itest_size = max(1000 // test_dataloader.batch_size, 1)
    for epoch in range(epochs):
        train_loss = torch.zeros((), device=device)
        itrain_loss = 0.0
        model.train()
        elements = None
        if hasattr(train_dataloader.sampler, "set_epoch"):
            train_dataloader.sampler.set_epoch(epoch)  # DistributedSampler: a new shuffle per epoch
        for batch, tup in enumerate(train_dataloader):
            elements = _to_device(tup, model)
            loss = get_loss(loss_fn, model, elements)
            optimizer.zero_grad()
            loss.backward()  # gradient all-reduce buckets start inside (ddp.OverlappedReducer)
            reducer.finish()
            optimizer.step()
            train_loss += loss.detach()
            if iteration_loss_frequency and batch and batch % iteration_loss_frequency == 0:
                itrain_losses.append((train_loss.item() - itrain_loss) / iteration_loss_frequency)
                itrain_loss = train_loss.item()
                itest_losses.append(_evaluate(model, loss_fn, test_dataloader, elements if stale_eval else None,
                                              itest_size) / itest_size)
                model.train()
        if mining:
            mined_fraction.append(loss_fn.mined_fraction())
        if with_memory:
            memory_fraction.append(loss_fn.memory_fraction())
        if contrastive:
            positive_probability.append(loss_fn.positive_probability())
        test_loss = _evaluate(model, loss_fn, test_dataloader, elements if stale_eval else None, None)
        train_losses.append(train_loss.item() / max(len(train_dataloader), 1))
        test_losses.append(test_loss / max(len(test_dataloader), 1))
        print(f"Epoch {epoch+1} - Train loss: {train_losses[epoch]:.5f} | Test loss: {test_losses[epoch]:.5f}",
              flush=True)
    out = {"train_losses": train_losses, "test_losses": test_losses, "itrain_losses": itrain_losses,
           "itest_losses": itest_losses, "iteration_loss_frequency": iteration_loss_frequency,
           "iteration_test_size": itest_size, "training_time": timer() - start_time}
    if mining:
        out["mined_fraction"] = mined_fraction
    if with_memory:
        out["memory_fraction"] = memory_fraction
    if contrastive:
        out["positive_probability"] = positive_probability
    return out


def _to_device(tup, model):
    """one collated batch on the GPU: tensors are moved; with --gpu_preprocess the
    images arrive as lists of decoded uint8 pixels and each branch is transformed
    by ONE library call (preprocess.ClipPreprocess: Resize bicubic, CenterCrop,
    RGB, ToTensor, Normalize of models.py:289-295, bit-identical to the CPU path)"""
    import preprocess
    res = getattr(model, "input_resolution", 224)
    return [preprocess.to_device_batch(e, res, device) if isinstance(e, list) else e.to(device) for e in tup]


@torch.no_grad()
def _evaluate(model, loss_fn, loader, stale, limit):
    """eval-mode loss over the test batches (or over the stale train batch, as the reference)."""
    ddp.broadcast_buffers(model)  # eval BatchNorm with rank 0's running statistics (torch DDP semantics)
    model.eval()
    total = 0.0
    for b, tup in enumerate(loader):
        el = stale if stale is not None else _to_device(tup, model)
        total += float(get_loss(loss_fn, model, el).item())
        if limit is not None and b >= limit:
            break
    return total


def make_loss(loss_type, with_classification, dataset_name, margin, negatives='given', memory_size=0,
              temperature=None, gather_negatives=False):
    """the reference's loss for the configuration; negatives 'hardest' / 'semihard' wraps
    it in losses.MinedNegatives with the metric of loss_type, 'all' gives losses.InfoNCELoss
    at `temperature` (default 0.07) instead; memory_size > 0 gives either a
    losses.CrossBatchMemory of memory_size rows (of the embeddings' width, allocated at the
    first step); gather_negatives (with 'all') makes every rank's rows of the step the
    loss's candidates (losses.InfoNCELoss(gather=True); no effect at one rank)"""
    _check_memory_size(memory_size, negatives)
    _check_contrastive(negatives, temperature, loss_type, with_classification)
    _check_gather(gather_negatives, negatives)
    memory = losses.CrossBatchMemory(memory_size, None) if memory_size else None
    if negatives == 'all':
        return losses.InfoNCELoss(DEFAULT_TEMPERATURE if temperature is None else temperature, memory=memory,
                                  gather=bool(gather_negatives))
    loss_fn = _make_loss(loss_type, with_classification, dataset_name, margin)
    if negatives == 'given':
        return loss_fn
    return losses.MinedNegatives(loss_fn, mode=negatives, metric=loss_type, memory=memory)


def _check_memory_size(memory_size, negatives):
    if memory_size < 0:
        raise SystemExit(f"--memory_size {memory_size} must be >= 0")
    if memory_size and negatives == 'given':
        raise SystemExit("--memory_size needs --negatives hardest or semihard: the memory only adds candidates "
                         "to the mining")


def _check_gather(gather_negatives, negatives):
    if gather_negatives and negatives != 'all':
        raise SystemExit("--gather_negatives needs --negatives all: only the InfoNCE loss takes the rows of every "
                         "rank as candidates (the mined triplet losses stay in their shard)")


DEFAULT_TEMPERATURE = 0.07


def _check_contrastive(negatives, temperature, loss_type=None, with_classification=False):
    """--negatives all / --temperature; loss_type None: not known yet (parse time checks it
    from the arguments)"""
    if negatives != 'all':
        if temperature is not None:
            raise SystemExit("--temperature needs --negatives all: only the InfoNCE loss has a temperature")
        return
    if temperature is not None and not temperature > 0:
        raise SystemExit(f"--temperature {temperature} must be > 0")
    if loss_type is not None and loss_type != 'cosine':
        raise SystemExit("--negatives all needs --loss_type cosine: the InfoNCE loss trains the cosine similarity, "
                         "and inference must rank by the similarity that was trained")
    if with_classification:
        raise SystemExit("--negatives all needs a model without classification heads: the InfoNCE loss is not "
                         "combined with the classification composites")


def _make_loss(loss_type, with_classification, dataset_name, margin):
    if loss_type == 'euclidean':
        if with_classification:
            if 'Sketchy' in dataset_name:
                return utils.TripletMarginLoss_with_classification(margin=margin)
            if 'Mixed' in dataset_name:
                return utils.TripletMarginLoss_with_classification(margin=margin, classification_weight=0.01)
            if 'Kaggle' in dataset_name:
                return utils.TripletMarginLoss_with_classification2(margin=margin, classification_weight=0,
                                                                    classification_weight2=0.2)
        return losses.TripletMarginLoss(margin=margin)
    if loss_type == 'cosine':
        if with_classification:
            if 'Kaggle' in dataset_name:
                return utils.TripletMarginLoss_with_classification2(margin=margin, distance_f=utils.cosine_distance)
            return utils.TripletMarginLoss_with_classification(margin=margin, distance_f=utils.cosine_distance)
        return losses.TripletMarginWithDistanceLoss(margin=margin, distance_function=utils.cosine_distance)
    raise Exception(f"loss type not correct {loss_type}")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Starts training a model")
    p.add_argument("-e", "--epochs", type=int, default=1)
    p.add_argument("-b", "--batch_size", type=int, default=32)
    p.add_argument("-l", "--learning_rate", type=float, default=0.00001)
    p.add_argument("-m", "--model", type=str, default='openResNet50m.pth')
    p.add_argument('--model_type', type=str, default='ModifiedResNet',
                   choices=['ModifiedResNet', 'ModifiedResNet_with_classification', 'VisionTransformer'])
    p.add_argument("-d", "--dataset", type=str, default='Synthetic')
    p.add_argument("-s", "--dsize", type=float, default=1.0)
    p.add_argument("--inference", action="store_true")
    p.add_argument('--feature_folder', default=None)
    p.add_argument("--no_training", action='store_true')
    p.add_argument("-w", "--weight_decay", type=float, default=0.002)
    p.add_argument('--img_type', type=str, default='photos')
    p.add_argument('--sketch_type', default='sketches_png')
    p.add_argument('--sketch_format', default='png', choices=['png', 'jpg'])
    p.add_argument('--loss_type', default='euclidean', choices=['euclidean', 'cosine'])
    p.add_argument('--loss_margin', type=float, default=0.2)
    # additions
    p.add_argument('--dtype', default='f32', choices=['f32', 'bf16', 'fp8'],
                   help="encoder compute dtype (fp8: the ViT's projection GEMMs)")
    p.add_argument('--layers', default='3,4,6,3', help="ModifiedResNet layers (reference: 3,4,6,3)")
    p.add_argument('--output_dim', type=int, default=1024)
    p.add_argument('--resolution', type=int, default=224)
    p.add_argument('--width', type=int, default=64)
    p.add_argument('--vit_width', type=int, default=768, help="VisionTransformer width (ViT-B/16: 768)")
    p.add_argument('--vit_layers', type=int, default=12, help="VisionTransformer blocks (ViT-B/16: 12)")
    p.add_argument('--patch_size', type=int, default=16, help="VisionTransformer patch size (ViT-B/16: 16)")
    p.add_argument('--data_pixels', action='store_true',
                   help="synthetic datasets as decoded image files of varied sizes (or the files, if present) "
                        "through the model's CPU transform in the DataLoader workers, as the reference")
    p.add_argument('--gpu_preprocess', action='store_true',
                   help="DataLoader workers only decode; the transform runs on the GPU per batch "
                        "(preprocess.ClipPreprocess; implies --data_pixels)")
    p.add_argument('--workers', type=int, default=None, help="DataLoader workers (reference: min(4, cpus))")
    p.add_argument('--synthetic_n', type=int, default=256, help="triplets in the synthetic dataset")
    p.add_argument('--stale_eval', dest='stale_eval', action='store_true', default=True,
                   help="the reference's test loss on the stale last train batch (train.py:80,89; default)")
    p.add_argument('--fresh_eval', dest='stale_eval', action='store_false',
                   help="test loss over the test batches instead of the stale train batch")
    p.add_argument('--no_save', action='store_true')
    p.add_argument('--negatives', default='given', choices=['given', 'hardest', 'semihard', 'all'],
                   help="the negative of every triplet: the one the dataset drew (the reference), or mined among "
                        "the 2 x batch gallery-side embeddings of the step (losses.MinedNegatives; per process "
                        "under torch.distributed.run: the step's candidates are not exchanged between ranks, "
                        "--memory_size adds past rows of every rank); all: every one of them, by the InfoNCE "
                        "loss (losses.InfoNCELoss; needs --loss_type cosine and no classification heads; "
                        "--gather_negatives adds the step's rows of every other rank)")
    p.add_argument('--temperature', type=float, default=None,
                   help="temperature of the InfoNCE loss (--negatives all; default 0.07)")
    p.add_argument('--memory_size', type=int, default=0,
                   help="cross-batch memory: also mine among the last M gallery-side embeddings of earlier steps, "
                        "of every rank under torch.distributed.run (losses.CrossBatchMemory; 0 = off; needs "
                        "--negatives hardest or semihard)")
    p.add_argument('--gather_negatives', action='store_true',
                   help="--negatives all under torch.distributed.run: the candidates of the InfoNCE loss are the "
                        "gallery-side embeddings of every rank, gathered in the forward, their gradients summed and "
                        "returned to their rank in the backward (no effect in one process)")
    args = p.parse_args(argv)
    _check_gather(args.gather_negatives, args.negatives)
    _check_memory_size(args.memory_size, args.negatives)
    _check_contrastive(args.negatives, args.temperature, args.loss_type, 'with_classification' in args.model_type)
    if args.negatives == 'all' and args.temperature is None:
        args.temperature = DEFAULT_TEMPERATURE
    return args


def main(argv=None):
    args = parse_args(argv)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        ddp.init_distributed()
    utils.MARGIN = args.loss_margin
    layers = tuple(int(v) for v in args.layers.split(","))
    model = utils.build_model(args.dataset, args.model_type, layers=layers, output_dim=args.output_dim,
                              input_resolution=args.resolution, width=args.width, heads=args.width * 32 // 64,
                              vit_width=args.vit_width, vit_layers=args.vit_layers, patch_size=args.patch_size)
    if os.path.isfile(os.path.join("models", args.model)):
        model = utils.load_model(args.model, dataset=args.dataset, model_type=args.model_type)
    model.freeze_layers()
    model.compute_dtype = {"bf16": torch.bfloat16, "f32": torch.float32, "fp8": "fp8"}[args.dtype]
    if args.dtype == "fp8" and not isinstance(model, models.VisionTransformer):
        raise SystemExit("--dtype fp8 applies to the ViT encoder (--model_type VisionTransformer)")
    model.to(device)
    ddp.broadcast_parameters(model)
    train_dataset, test_dataset = data_preparation.get_datasets(dataset=args.dataset, size=args.dsize,
                                                                transform=model.transform, n=args.synthetic_n,
                                                                resolution=args.resolution,
                                                                pixels=args.data_pixels or args.gpu_preprocess,
                                                                decode_only=args.gpu_preprocess,
                                                                ids=args.negatives != 'given')
    sampler = None
    if world > 1:
        sampler = torch.utils.data.distributed.DistributedSampler(train_dataset, shuffle=True)
    workers = args.workers if args.workers is not None else min(4, os.cpu_count())  # train.py:154-155
    collate = data_preparation.collate_decoded if args.gpu_preprocess else None
    train_loader = DataLoader(train_dataset, batch_size=args.batch_size, num_workers=workers,
                              shuffle=sampler is None, sampler=sampler, collate_fn=collate,
                              pin_memory=torch.cuda.is_available() and not args.gpu_preprocess)
    test_loader = DataLoader(test_dataset, batch_size=args.batch_size, num_workers=workers, shuffle=False,
                             collate_fn=collate)
    optimizer = optim.Adam(model.parameters(), lr=args.learning_rate, weight_decay=args.weight_decay)
    with_classification = 'with_classification' in type(model).__name__ and 'V2' in train_dataset.state_dict['dataset']
    loss_fn = make_loss(args.loss_type, with_classification, train_dataset.state_dict['dataset'], utils.MARGIN,
                        args.negatives, args.memory_size, args.temperature, gather_negatives=args.gather_negatives)
    param_dict = {"model": args.model, "trained_layers": model.trained_layers, "dataset": args.dataset,
                  "epochs": args.epochs, "batch_size": args.batch_size, "learning_rate": args.learning_rate,
                  "weight_decay": args.weight_decay, "optimizer": type(optimizer).__name__,
                  "loss_fn": type(loss_fn).__name__, "loss_margin": loss_fn.margin, "loss_type": args.loss_type,
                  "dtype": args.dtype}
    if args.negatives != 'given':
        param_dict["negatives"] = args.negatives
    if args.negatives == 'all':
        param_dict["temperature"] = args.temperature
    if args.memory_size:
        param_dict["memory_size"] = args.memory_size
    if args.gather_negatives:
        param_dict["gather_negatives"] = True
    data_dict = train_dataset.state_dict
    print(param_dict, flush=True)
    print(data_dict, flush=True)
    training_dict, inference_dict = {}, {}
    if not args.no_training:
        training_dict = triplet_train(model, args.epochs, train_loader, test_loader, loss_fn, optimizer,
                                      with_classification, stale_eval=args.stale_eval)
    rank0 = int(os.environ.get("RANK", "0")) == 0
    if args.inference:
        # every rank takes part: with several processes the gallery embedding
        # and the retrieval are sharded over them (collectives), and all ranks
        # embed with rank 0's BatchNorm running statistics (DDP broadcast_buffers)
        ddp.broadcast_buffers(model)
        inference_dict = inference.run_inference(model, test_dataset, args.feature_folder, args.loss_type)
        if rank0:
            print({k: v for k, v in inference_dict.items() if k != "retrieval_samples"}, flush=True)
    if rank0 and not args.no_save:
        folder = utils.save_model(model, data_dict, training_dict, param_dict, inference_dict)
        visualization.visualize(folder, training_dict, inference_dict)  # train.py:195
    return training_dict, inference_dict


if __name__ == "__main__":
    main()
