#!/usr/bin/env python3
"""Whole-radargram segmentation drivers -- the reference's scripts/test/test_mc1.py, test_mc3.py and test_sharad.py behind one
entry point (``--driver``), same flags and defaults, same input files, same output files (``torch.save``); the PNG plots are
not drawn.  The segmentation itself is ``inference.segment_radargrams``.

    python radar-sounder-crw_amd/scripts/segment_drivers.py --driver mc3 --model_path latestx.pt \\
        --input_folder resources/input/ --output_folder resources/output/

Additions: ``--model_path`` (the scripts hard-code their checkpoints; a state_dict with or without DataParallel's ``module.``
prefix), ``--model`` (0 = CNN, 1 = Resnet, the scripts' choice), ``--change_idx`` (mc3 / sharad's hand-set change points).
Differences: ``--use_last`` / ``--correction`` read true / false (the scripts take any given string as true), ``--patch_size``
takes two numbers, and the folders default to ``resources/input/`` / ``resources/output/`` under the working directory.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from inference import DRIVERS, segment_radargrams
from utils import create_model


def _flag(s):
    v = str(s).strip().lower()
    if v in ('1', 'true', 'yes', 'on'):
        return True
    if v in ('0', 'false', 'no', 'off'):
        return False
    raise argparse.ArgumentTypeError(f'expected true / false, got {s!r}')


def _change(s):
    return None if s.lower() == 'none' else int(s)


def get_args_parser():
    p = argparse.ArgumentParser('CRW whole-radargram drivers (MC1 / MC3 / SHARAD)', add_help=True)
    p.add_argument('--driver', required=True, choices=sorted(DRIVERS))
    p.add_argument('--patch_size', default=None, nargs=2, type=int)
    p.add_argument('--seq_length', default=None, type=int)
    p.add_argument('--overlap', default=None, nargs='+', type=int)
    p.add_argument('-c', '--cxt_size', default=None, type=int)
    p.add_argument('-r', '--radius', default=None, type=int)
    p.add_argument('-t', '--temp', default=None, type=float)
    p.add_argument('-k', '--knn', default=None, type=int)
    p.add_argument('--context', default='reference', choices=('reference', 'sliding'),
                   help="frames a late frame's neighbour indices address: the reference's rule, or the frames they were scored on")
    p.add_argument('--use_last', default=None, type=_flag, help='reverse pass (mc1 / mc3; sharad never reads it)')
    p.add_argument('--correction', default=None, type=_flag, help='correction step (mc3; sharad always corrects, mc1 never)')
    p.add_argument('--change_idx', default=None, nargs=3, type=_change, help='hand-set change points of the three radargrams')
    p.add_argument('--model', default=None, type=int, help='0 = CNN, 1 = Resnet')
    p.add_argument('--model_path', required=True, help='encoder state_dict (the scripts: latestx.pt / sharad16_3.pt)')
    p.add_argument('--input_folder', default='resources/input/')
    p.add_argument('--output_folder', default='resources/output/')
    return p


def with_defaults(args):
    """Fill every flag left unset with the driver's default (inference.DRIVERS)."""
    d = DRIVERS[args.driver]
    for k in ('patch_size', 'seq_length', 'overlap', 'cxt_size', 'radius', 'temp', 'knn', 'use_last', 'correction', 'change_idx',
              'model'):
        if getattr(args, k) is None:
            setattr(args, k, d[k])
    args.patch_size, args.overlap = tuple(args.patch_size), tuple(args.overlap)
    args.change_idx = None if args.change_idx is None else tuple(args.change_idx)
    return args


def load_inputs(driver, folder, device):
    """The scripts' input files, with their casts and edits -> (radargrams, references, reversed references or None)."""
    ld = lambda name: torch.load(os.path.join(folder, name), map_location='cpu')
    if driver == 'mc1':  # test_mc1.py:54-65
        rg = [ld(f'mc1_{i}.pt').to(device) for i in (1, 2, 3)]
        sg = [ld(f'mc1_{i}ref.pt').to(device) for i in (1, 2, 3)]
        sgr = [ld(f'mc1_{i}ref_r.pt').to(device) for i in (1, 2, 3)]
        return rg, sg, sgr
    if driver == 'mc3':  # test_mc3.py:54-61
        rg = [ld(n).float().to(device) for n in ('mc3_1.pt', 'mc3_2.pt', 'mc3_3y.pt')]
        sg = [ld(n).to(device) for n in ('mc3_1ref.pt', 'mc3_2ref.pt', 'mc3_3refy.pt')]
        sg[1][870:900, 1132:1200] = 2
        return rg, sg, None
    if driver == 'sharad':  # test_sharad.py:54-61
        rg = [ld(n).float().to(device) for n in ('s_1.pt', 's_4.pt', 's_3.pt')]
        sg = [ld(n).to(device) for n in ('s_1ref.pt', 's_4ref.pt', 's_3ref.pt')]
        rg[0], sg[0] = torch.flip(rg[0], dims=(1,)), torch.flip(sg[0], dims=(1,))
        return rg, sg, None
    raise ValueError(f'unknown driver {driver!r}')


def load_encoder(model, path, device):
    """create_model(model) with the checkpoint's weights; DataParallel's ``module.`` prefix is dropped if present.  Left in
    train mode, as the scripts leave it (they never call .eval(): BatchNorm normalises with the batch's statistics)."""
    encoder = create_model(model, False).to(device)
    sd = torch.load(path, map_location=device)
    if sd and all(k.startswith('module.') for k in sd):
        sd = {k[len('module.'):]: v for k, v in sd.items()}
    encoder.load_state_dict(sd)
    return encoder


def main(args):
    args = with_defaults(args)
    device = torch.device('cuda' if torch.cuda.is_available() else 'cpu')
    encoder = load_encoder(args.model, args.model_path, device)
    rg, sg, sgr = load_inputs(args.driver, args.input_folder, device)
    out = segment_radargrams(args.driver, rg, sg, encoder, refs_reversed=sgr, patch_size=args.patch_size,
                             seq_length=args.seq_length, overlap=args.overlap, cxt_size=args.cxt_size, radius=args.radius,
                             temp=args.temp, knn=args.knn, use_last=args.use_last, correction=args.correction,
                             change_idx=args.change_idx, context=args.context)
    os.makedirs(args.output_folder, exist_ok=True)
    for name, obj in out.items():
        torch.save(obj, os.path.join(args.output_folder, name))
        print('wrote', os.path.join(args.output_folder, name))
    return out


if __name__ == '__main__':
    torch.manual_seed(11)  # the scripts seed at import (test_mc1.py:15)
    main(get_args_parser().parse_args())
