"""PROD/ProD_KD/utils/dpr_utils.py:80-92: the optimizer factory every PROD, MASTER, LEAD and CAPSTONE train script calls.
The two parameter groups ('bias' / 'LayerNorm.weight' never decay) are built inside the fused optimizers from the same
rule; the rest of the reference module is host-side checkpoint and evaluation plumbing and is not rebuilt here."""
from simxns_amd.optim import FusedAdamW, FusedLamb


def get_optimizer(args, model, lr=2e-5, weight_decay=0.0):
    if args.optimizer == "adamW":
        return FusedAdamW(model, lr=lr, eps=args.adam_epsilon, weight_decay=weight_decay)
    elif args.optimizer == "lamb":
        return FusedLamb(model, lr=lr, eps=args.adam_epsilon, weight_decay=weight_decay)
    else:
        raise Exception("optimizer {0} not recognized! Can only be lamb or adamW".format(args.optimizer))
