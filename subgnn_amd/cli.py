"""The shared prelude of the ``python -m subgnn_amd.X`` entry points that answer from a checkpoint: the arguments that name
the run, the model behind them, the ``-target`` lookup and the output file.  The model's modules are imported when a model is
opened, not when arguments are parsed."""
import os
from pathlib import Path

import torch

from . import config


def add_run_arguments(ap):
    ap.add_argument('-config_path', type=str, required=True)
    ap.add_argument('-project_root', type=str, default=None, help='overrides subgnn_amd.config.PROJECT_ROOT')
    ap.add_argument('-restoreModelPath', type=str, required=True, help='directory of a run: its hyperparams.json is used')
    ap.add_argument('-restoreModelName', type=str, default=None,
                    help='checkpoint file in -restoreModelPath (default: the best epoch*.ckpt, else last.ckpt)')


def require_positive(ap, args, names):
    """``ap.error`` for the first of the options ``names`` that is given and not positive."""
    for name in names:
        v = getattr(args, name)
        if v is not None and v <= 0:
            ap.error('-%s must be positive' % name)


def parse_splits(ap, text):
    """``train,val`` -> ('train', 'val'); ``ap.error`` for none or an unknown one."""
    from .neighbors import SPLITS
    splits = tuple(s for s in text.split(',') if s)
    if not splits or any(s not in SPLITS for s in splits):
        ap.error('-splits takes a comma-separated list of %s' % ', '.join(SPLITS))
    return splits


def open_predictor(args):
    """The ``Predictor`` of the run that the run arguments name."""
    from .predict import Predictor
    from .train_config import read_json
    if args.project_root:
        config.PROJECT_ROOT = Path(args.project_root)
    return Predictor.from_run(read_json(args.config_path), args.restoreModelPath, args.restoreModelName)


def label_index(p, name):
    """The class index of the label string ``name`` (None: no ``-target`` was given -> None)."""
    if name is None:
        return None
    if p.label_names is None or name not in p.label_names:
        raise SystemExit('-target: %r is no label of the dataset (%s)' % (name, p.label_names))
    return p.label_names.index(name)


def predicted_names(p, logits_row):
    """The label strings of one row of logits, as ``predict`` forms the labels."""
    return p.names_of(torch.sigmoid(logits_row) > 0.5 if p.model.multilabel else logits_row.argmax())


def write_lines(path, lines, header=None):
    with open(path, 'w') as f:
        if header is not None:
            f.write(header + '\n')
        for line in lines:
            f.write(line + '\n')


def open_index(p, args):
    """The ``SubgraphIndex`` of ``-index`` if that file exists (searched under ``-metric``), else the index of the model's
    ``-splits``, saved to ``-index`` if one is named."""
    from .neighbors import SubgraphIndex
    if args.index is not None and os.path.exists(args.index):
        index = SubgraphIndex.load(args.index, p.model.device, predictor=p)
        index.metric, index._aux = args.metric, None
    else:
        index = SubgraphIndex.from_predictor(p, args.splits, args.batch_size, args.metric)
        if args.index is not None:
            index.save(args.index)
    return index
