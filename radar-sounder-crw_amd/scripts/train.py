#!/usr/bin/env python3
"""CRW training entrypoint -- same flags and defaults as the reference's scripts/train.py:17-37
(--tune and the Ray-Tune branch are out of scope: third-party orchestration, SURVEY.md section 2
row 10).  Additions: --data_path / --synthetic H W (the reference's dataset paths are private),
--steps (stop early), --save (skip writing the checkpoint when empty), --shared_encode (a batch is
--batch_size CONSECUTIVE overlapping items whose patch-columns are encoded once, CRW.forward_columns).

Keeping a run alive (all opt-in; without these flags every output and printed line is what it was):
--nodata skip (items whose pixels hold a NaN or an infinity are left out of every epoch), --skip_nonfinite (a step whose
gradient is not finite is refused) and --clip_grad_norm X (the gradient's norm is bounded; implies the skip) through the guarded
Adam step of include/crw_hip_guard.h, --save_every N / --resume FILE (a checkpoint of encoder, optimizer and position every N steps).

Single GPU:   python radar-sounder-crw_amd/scripts/train.py --model 0 --synthetic 512 4096
Multi GPU:    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 \
                  radar-sounder-crw_amd/scripts/train.py --model 0 --synthetic 512 32768
One process per GPU; items (independent sequences) are sharded over ranks and the only exchange is
one RCCL all-reduce of the flat encoder gradient per step (the reference instead wraps the encoder
in nn.DataParallel and runs the walk on GPU 0, scripts/train.py:45-47).
"""
import argparse
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
from torch.optim import Adam
from torch.utils.data import DataLoader, Subset

from utils import create_model, create_dataset
from model import CRW
import dist as crw_dist

torch.manual_seed(11)

# the flags of this file that the reference does not have and that change nothing at their defaults: left out of the printed
# argument line while they are at their defaults, so that a run without them prints what it printed before they existed
SURVIVAL_DEFAULTS = dict(nodata='keep', clip_grad_norm=None, skip_nonfinite=False, save_every=0, resume='')


def get_args_parser():
    p = argparse.ArgumentParser('CRW Train', add_help=True)
    p.add_argument('--tune', default=False, type=bool, help='Ray Tune search (not supported here)')
    p.add_argument('--model', default=1, type=int, help='0=CNN,1=Resnet18')
    p.add_argument('--dataset', default=3, type=int, help='0=MCORDS1,1=Miguel,3=SHARAD')
    p.add_argument('--patch_size', default=(16, 16), nargs=2, type=int)
    p.add_argument('--seq_length', default=20, type=int)
    p.add_argument('--overlap', default=(8, 0), nargs='+', type=int)
    p.add_argument('--batch_size', default=8, type=int, help='global batch (items per step over all ranks)')
    p.add_argument('--epochs', default=2, type=int)
    p.add_argument('--lr', default=1E-3, type=float)
    p.add_argument('--tau', default=0.01, type=float)
    p.add_argument('--pos_embed', default=False, type=bool)
    p.add_argument('--dataset_full', default=True)
    p.add_argument('--output_folder', default='./resources/')
    p.add_argument('--output_name', default='sharad16_3')
    p.add_argument('--data_path', default=None, help='H x W radargram .pt file')
    p.add_argument('--synthetic', default=None, nargs=2, type=int, metavar=('H', 'W'))
    p.add_argument('--steps', default=0, type=int, help='stop after this many steps (0 = full epochs)')
    p.add_argument('--shared_encode', action='store_true',
                   help='batches of consecutive overlapping items share one encoder pass (needs --dataset_full)')
    p.add_argument('--host_data', action='store_true',
                   help='keep the radargram in host memory and feed items through a DataLoader like the reference '
                        '(default: the radargram lives on the GPU and items are cut there, no per-step H2D copy)')
    p.add_argument('--save', default='', help='checkpoint path for encoder.state_dict() (default: '
                                              '<output_folder>/models/<output_name>.pt)')
    p.add_argument('--nodata', default='keep', choices=('keep', 'skip'),
                   help="skip: items whose pixels hold a NaN or an infinity are left out of every epoch's order, the same on every "
                        'rank (with --shared_encode: a batch is dropped unless all its items are finite); keep: as they come')
    p.add_argument('--clip_grad_norm', default=None, type=float, metavar='X',
                   help="scale the gradient so that its norm is at most X (torch.nn.utils.clip_grad_norm_'s rule on an fp64 "
                        'norm); a clip implies --skip_nonfinite')
    p.add_argument('--skip_nonfinite', action='store_true',
                   help='refuse a step whose gradient holds a NaN or an infinity: parameters and moments stay as they are')
    p.add_argument('--save_every', default=0, type=int, metavar='N',
                   help='every N steps rank 0 writes <save>.ckpt: encoder, optimizer, epoch, step within the epoch, total step')
    p.add_argument('--resume', default='', metavar='FILE', help='continue from a checkpoint that --save_every wrote')
    return p


def printable(args):
    """args without the survival flags that are at their defaults (see SURVIVAL_DEFAULTS)"""
    kept = {k: v for k, v in vars(args).items() if k not in SURVIVAL_DEFAULTS or v != SURVIVAL_DEFAULTS[k]}
    return argparse.Namespace(**kept)


def check_flags(args):
    """the refusals of the survival flags, before anything is built -> True when the optimizer step is guarded"""
    for k, v in SURVIVAL_DEFAULTS.items():          # an args object from before the flags: their defaults
        if not hasattr(args, k):
            setattr(args, k, v)
    if args.nodata not in ('keep', 'skip'):
        raise SystemExit(f"--nodata must be 'keep' or 'skip' (got {args.nodata!r})")
    x = args.clip_grad_norm
    if x is not None and not (x > 0 and math.isfinite(x)):
        raise SystemExit(f'--clip_grad_norm must be a finite number > 0 (got {x})')
    if args.save_every < 0:
        raise SystemExit(f'--save_every must be >= 0 (got {args.save_every})')
    if args.resume and not os.path.isfile(args.resume):
        raise SystemExit(f'--resume {args.resume}: no such checkpoint')
    return x is not None or bool(args.skip_nonfinite)


def save_path(args):
    return args.save or os.path.join(args.output_folder, 'models', args.output_name + '.pt')


def finite_mask(dataset):
    """`RGDataset.finite_items()` of the dataset, or of the items a non-overlapping Subset keeps -> bool list"""
    if isinstance(dataset, Subset):
        keep = dataset.dataset.finite_items().cpu()
        return [bool(keep[i]) for i in dataset.indices]
    return dataset.finite_items().cpu().tolist()


def epoch_items(n_items, epoch, batch_size, finite=None):
    """-> (the epoch's item order cut to whole global batches, the epoch's generator).  The permutation is a function of the epoch
    number alone (identical on every rank, reproduced by a resumed run); with `finite` the items that are not are dropped from it
    before the batches are cut."""
    g = torch.Generator().manual_seed(11 + epoch)
    order = torch.randperm(n_items, generator=g).tolist()
    if finite is not None:
        order = [i for i in order if finite[i]]
    return order[:len(order) // batch_size * batch_size], g


def shared_batches(n_items, batch_size, g, finite=None):
    """--shared_encode: batch b = items [b * batch_size, (b + 1) * batch_size), the batch order shuffled per epoch; with `finite` a
    batch is dropped unless all of its items are finite"""
    nb = n_items // batch_size
    order = torch.randperm(nb, generator=g).tolist()
    if finite is not None:
        order = [b for b in order if all(finite[b * batch_size:(b + 1) * batch_size])]
    return order


class GuardedTorchAdam:
    """The CPU fallback of the guarded step: torch.optim.Adam behind torch.nn.utils.clip_grad_norm_ and an isfinite test, with
    the counters of `optim.FlatAdam.stats()`.  A refused step does not reach the optimizer, so its step count -- and with it the
    bias corrections -- counts applied steps only."""

    def __init__(self, params, lr, max_grad_norm=None, skip_nonfinite=False):
        self.params = [p for p in params if p.requires_grad]
        self.opt = Adam(self.params, lr=lr)
        self.max_grad_norm, self.skip_nonfinite = max_grad_norm, skip_nonfinite
        self.guarded = max_grad_norm is not None or skip_nonfinite
        self.counts = dict(applied=0, skipped=0, last_norm=0.0, last_scale=0.0, last_applied=0)

    def step(self):
        if not self.guarded:
            self.opt.step()
            return
        grads = [p.grad for p in self.params if p.grad is not None]
        norm = float(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g.double()) for g in grads])))
        c = self.counts
        if not math.isfinite(norm):
            c.update(skipped=c['skipped'] + 1, last_norm=norm, last_scale=0.0, last_applied=0)
            return
        scale = 1.0
        if self.max_grad_norm is not None:
            torch.nn.utils.clip_grad_norm_(self.params, self.max_grad_norm)
            scale = min(1.0, self.max_grad_norm / (norm + 1e-6))
        self.opt.step()
        c.update(applied=c['applied'] + 1, last_norm=norm, last_scale=scale, last_applied=1)

    def stats(self):
        return dict(self.counts)

    def state_dict(self):
        return {'adam': self.opt.state_dict(), 'counts': dict(self.counts)}

    def load_state_dict(self, sd):
        self.opt.load_state_dict(sd['adam'])
        self.counts.update(sd['counts'])


def save_checkpoint(path, encoder, optimizer, epoch, step_in_epoch, total_step):
    """<save>.ckpt: everything a resumed run needs.  Written beside the target and moved over it, so that a run killed while
    writing leaves the previous checkpoint whole."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    tmp = path + '.tmp'
    torch.save({'encoder': encoder.state_dict(), 'optimizer': optimizer.state_dict(), 'epoch': int(epoch),
                'step_in_epoch': int(step_in_epoch), 'total_step': int(total_step)}, tmp)
    os.replace(tmp, path)


def load_checkpoint(path, encoder, optimizer, device='cpu'):
    """-> (epoch, step_in_epoch, total_step).  The encoder's parameters are copied in place (they stay views of a flat buffer)."""
    ck = torch.load(path, map_location=device)
    encoder.load_state_dict(ck['encoder'])
    optimizer.load_state_dict(ck['optimizer'])
    return int(ck['epoch']), int(ck['step_in_epoch']), int(ck['total_step'])


def main(args, on_step=None):
    """on_step(step_index, loss): optional observer called after every optimizer step with the step's (detached, on-device)
    loss of this rank.  After the run `main.optimizer` is the optimizer it used (its `stats()`, for a guarded one)."""
    rank, world, local = crw_dist.init_from_env()
    guarded = check_flags(args)
    if rank == 0:
        print(printable(args))
    if args.tune:
        raise SystemExit('--tune (Ray Tune) is outside the scope of the MI355X build')
    device = torch.device('cuda', local)
    torch.cuda.set_device(device)

    encoder = create_model(args.model, args.pos_embed)  # same seed on every rank -> identical replicas
    model = CRW(encoder, args.tau, args.pos_embed).to(device)
    dataset = create_dataset(id=args.dataset, length=args.seq_length, dim=tuple(args.patch_size),
                             full=args.dataset_full, overlap=tuple(args.overlap), data_path=args.data_path,
                             synthetic=args.synthetic)
    if args.batch_size % world:
        raise SystemExit(f'--batch_size {args.batch_size} must be a multiple of the number of ranks ({world})')
    per_rank = args.batch_size // world
    # Like a DataLoader with drop_last=True the tail of an epoch that does not fill a global batch is dropped (the
    # reference's loader keeps a final partial batch, scripts/train.py:53): equal shards per rank are what make the mean of
    # the rank gradients the global gradient.  A dataset shorter than one batch would silently train nothing: refuse it.
    if len(dataset) < args.batch_size:
        raise SystemExit(f'the dataset holds {len(dataset)} items, fewer than one global batch (--batch_size {args.batch_size}): '
                         'no step would run; lower --batch_size or --seq_length, or use a longer radargram')
    if args.shared_encode and not hasattr(dataset, 'columns'):
        raise SystemExit('--shared_encode needs the overlapping dataset (--dataset_full True)')

    base = dataset.dataset if isinstance(dataset, Subset) else dataset
    if not args.host_data:
        # the item cut is a strided view of the radargram (src/dataset.py:19-39): with the radargram resident in
        # HBM a batch is one gather kernel instead of a CPU unfold + 16 MB host-to-device copy per step
        base.T = base.T.to(device)
    finite = None
    if args.nodata == 'skip':
        finite = finite_mask(dataset)
        if args.shared_encode:
            left = len(shared_batches(len(dataset), args.batch_size, torch.Generator().manual_seed(0), finite)) * args.batch_size
        else:
            left = sum(finite)
        if rank == 0:
            print(f'--nodata skip: {len(finite) - sum(finite)} of {len(finite)} items hold a NaN or an infinity; '
                  f'{len(dataset) - left} items are left out of every epoch')
        if left < args.batch_size:
            raise SystemExit(f'the dataset holds {left} finite items, fewer than one global batch (--batch_size {args.batch_size}): '
                             'no step would run; lower --batch_size or --seq_length, or use a longer radargram')
    bucket = crw_dist.FlatGradBucket(model.parameters(), lazy=True)
    if device.type == "cuda":  # torch.optim.Adam's update (the reference's optimizer) as one launch over flat buffers
        import optim as crw_optim
        optimizer = crw_optim.FlatAdam(bucket, lr=args.lr, max_grad_norm=args.clip_grad_norm, skip_nonfinite=args.skip_nonfinite) \
            if guarded else crw_optim.FlatAdam(bucket, lr=args.lr)
    else:
        optimizer = GuardedTorchAdam(model.parameters(), args.lr, args.clip_grad_norm, args.skip_nonfinite) if guarded else \
            Adam(model.parameters(), lr=args.lr)
    main.optimizer = optimizer
    first_epoch = consumed = nsteps = 0
    if args.resume:
        first_epoch, consumed, nsteps = load_checkpoint(args.resume, encoder, optimizer, device)
        if rank == 0:
            print(f'Resumed {args.resume}: epoch {first_epoch}, {consumed} steps into it, {nsteps} steps in all')
    model.train(True)
    loss_tot = []
    for epoch in range(first_epoch, args.epochs):
        t0 = time.time()
        order, g = epoch_items(len(dataset), epoch, args.batch_size, finite)  # identical permutation on every rank
        skip = consumed if epoch == first_epoch else 0                         # a resumed epoch: the batches it already took
        mine = [order[i] for i in range(len(order)) if (i % args.batch_size) // per_rank == rank][skip * per_rank:]
        if args.shared_encode:
            # batch b = items [b*batch_size, (b+1)*batch_size): rank r walks per_rank consecutive items whose
            # per_rank + seq_length - 1 patch-columns are encoded once; batch order is shuffled per epoch
            loader = (dataset.columns(b * args.batch_size + rank * per_rank, per_rank + args.seq_length - 1)[None]
                      for b in shared_batches(len(dataset), args.batch_size, g, finite)[skip:])
        elif args.host_data:
            loader = DataLoader(Subset(dataset, mine), batch_size=per_rank, shuffle=False)
        else:
            loader = (torch.stack([dataset[i] for i in mine[b:b + per_rank]])
                      for b in range(0, len(mine) - per_rank + 1, per_rank))
        loss_epoch = []
        for seq in loader:
            seq = seq.to(device, non_blocking=True)
            bucket.zero()
            loss, _ = model.forward_columns(seq, args.seq_length) if args.shared_encode else model(seq)
            loss.backward()
            bucket.all_reduce_mean()
            optimizer.step()
            loss_epoch.append(loss.detach())
            nsteps += 1
            if on_step is not None:
                on_step(nsteps, loss_epoch[-1])
            if args.save_every and nsteps % args.save_every == 0 and rank == 0:
                save_checkpoint(save_path(args) + '.ckpt', encoder, optimizer, epoch, skip + len(loss_epoch), nsteps)
            if args.steps and nsteps >= args.steps:
                break
        if skip and not loss_epoch:  # resumed at the very end of an epoch: nothing of it is left to report
            continue
        if loss_epoch and guarded:  # the loss of a refused step is not a number: the epoch's mean is over the others
            losses = torch.stack(loss_epoch)
            ok = torch.isfinite(losses)
            mean = torch.where(ok, losses, torch.zeros_like(losses)).sum() / ok.sum().clamp_min(1)
        else:
            mean = torch.stack(loss_epoch).mean() if loss_epoch else torch.zeros((), device=device)
        if world > 1:
            torch.distributed.all_reduce(mean, op=torch.distributed.ReduceOp.SUM)
            mean /= world
        loss_tot.append(mean.item())
        cols = len(loss_epoch) * args.batch_size * (args.seq_length * (args.patch_size[1] - args.overlap[1])
                                                   + args.overlap[1])
        if rank == 0:
            dt = time.time() - t0
            line = ('Epoch:', epoch, 'Loss:', loss_tot[-1], 'Time:', dt, 'columns/s:', cols / max(dt, 1e-9))
            if guarded:
                st = optimizer.stats()
                line += ('skipped:', st['skipped'], ' grad norm:', st['last_norm'])
            print(*line)
        if args.steps and nsteps >= args.steps:
            break

    if rank == 0:
        path = save_path(args)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        torch.save(encoder.state_dict(), path)
        print('Finished training.')
    if world > 1:
        torch.distributed.destroy_process_group()
    return loss_tot


if __name__ == '__main__':
    a = get_args_parser().parse_args()
    a.overlap = tuple(a.overlap)
    main(a)
