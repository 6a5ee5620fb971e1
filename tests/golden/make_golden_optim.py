#!/usr/bin/env python3
"""Golden values for the host half of aoc_amd.optim_train (tests/test_optim_host.py), recorded by running the reference's OWN
``utils/learning.py`` UNMODIFIED (it imports only ``math``): ``adjust_learning_rate`` and ``get_trainable_params``.  None of the reference's
text is stored, and nothing is written into its tree.  Neither ``DeepLab`` nor ``ResNet101`` is constructed (their default path fetches
weights); the groups are recorded for the toy module below.

Recorded in optim_schedule.json:

    schedule   the learning rate at steps 0, 1, 999, 1000, 1001, 25 000, 49 999 and 50 000 of the committed configuration (TRAIN_LR 0.01, power
               0.9, warm-up 1000, 50 000 steps), polynomial and cosine, with the default ``min_lr`` and with one the floor holds for mid-run;
               each value as ``float.hex`` (exact) and as a decimal for the reader
    groups     what ``get_trainable_params`` returns for the toy module, ``beta_wd`` both ways: the parameter's name, ``weight_decay``, ``lr``

    python tests/golden/make_golden_optim.py <the reference's complete_project/AOCNet directory>
"""
import importlib.util
import json
import os
import sys

import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True                            # never write into the reference tree

STEPS = (0, 1, 999, 1000, 1001, 25000, 49999, 50000)
BASE_LR, POWER, WARM_UP, TOTAL = 0.01, 0.9, 1000, 50000


class _Gate(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.alpha, self.gamma, self.beta = nn.Parameter(torch.ones(1, c, 1, 1)), nn.Parameter(torch.zeros(1, c, 1, 1)), nn.Parameter(torch.zeros(1, c, 1, 1))


class Toy(nn.Module):
    """a convolution, two GCT-shaped gates (alpha, gamma, beta), a GroupNorm and one frozen parameter"""

    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(3, 4, 1)
        self.gct = _Gate(4)
        self.block = nn.Sequential(nn.GroupNorm(2, 4), _Gate(4))
        self.frozen = nn.Parameter(torch.zeros(5), requires_grad=False)


class _Opt:
    def __init__(self):
        self.param_groups = [{"lr": None}, {"lr": None}]


def main(ref_root):
    spec = importlib.util.spec_from_file_location("ref_learning", os.path.join(ref_root, "utils", "learning.py"))
    learning = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(learning)                                       # the reference's file, unmodified
    schedule = []
    for cosine in (False, True):
        for kwargs in ({}, {"min_lr": 4e-3}):
            for itr in STEPS:
                opt = _Opt()
                lr = learning.adjust_learning_rate(opt, BASE_LR, POWER, itr, TOTAL, WARM_UP, cosine, **kwargs)
                assert all(g["lr"] == lr for g in opt.param_groups)
                schedule.append(dict(base_lr=BASE_LR, p=POWER, itr=itr, max_itr=TOTAL, warm_up_steps=WARM_UP, is_cosine_decay=cosine,
                                     min_lr=kwargs.get("min_lr"), lr_hex=float(lr).hex(), lr=float(lr), floored=bool(lr == kwargs.get("min_lr", 1e-5))))
    assert any(s["floored"] and s["min_lr"] and 1000 < s["itr"] < 50000 for s in schedule), "no case in which the min_lr floor holds mid-run"
    torch.manual_seed(0)
    toy = Toy()
    names = {id(p): n for n, p in toy.named_parameters()}
    groups = {}
    for beta_wd in (True, False):
        got = learning.get_trainable_params(toy, BASE_LR, 1e-4, beta_wd)
        groups[str(beta_wd)] = [dict(names=[names[id(p)] for p in g["params"]], weight_decay=g["weight_decay"], lr=g["lr"]) for g in got]
    out = dict(schedule=schedule, toy=[[n, list(p.shape), bool(p.requires_grad)] for n, p in toy.named_parameters()], base_lr=BASE_LR, weight_decay=1e-4,
               groups=groups)
    path = os.path.join(HERE, "optim_schedule.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{path}: {os.path.getsize(path)} bytes, {len(schedule)} schedule points, {sum(s['floored'] for s in schedule)} floored")


if __name__ == "__main__":
    main(os.path.abspath(sys.argv[1]))
