"""Dataset half of the reference config (own restatement of open_loop_training/configs/thinktwice.py:5-33, :64-108; cited per
field): which towns train and validate, the per-town sample caps, the frame queue and the label classes.  Pure data."""
import copy

from . import calib

_TOWN_IDS = ("01", "02", "03", "04", "05", "06", "07", "10")
INDEX_PER_TOWN = ["val"] + [str(i).zfill(2) for i in range(12)]                       # CFG:12

DEV_MAX_SAMPLE_PER_TOWN = {"town" + t: 10 for t in _TOWN_IDS}                         # CFG:5
DEV_TRAIN = ["town01_00"]                                                             # CFG:6
DEV_VAL = ["town01_00"]                                                               # CFG:7

TCP_MAX_SAMPLE_PER_TOWN = {"town01": 50384, "town02": 55943, "town03": 42771, "town04": 47954, "town05": 53684,
                           "town06": 48415, "town07": 51549, "town10": 59898}         # CFG:9
TCP_TRAIN = ["town" + t + "_" + i for t in ("01", "03", "04", "06") for i in INDEX_PER_TOWN]      # CFG:10, :14-17
TCP_VAL = ["town" + t + "_" + i for t in ("02", "05") for i in INDEX_PER_TOWN]                    # CFG:11, :19-22

FULL_TRAIN = ["town" + t + "_" + i for t in _TOWN_IDS for i in INDEX_PER_TOWN if i != "val"]      # CFG:24-32
FULL_VAL = ["town" + t + "_val" for t in _TOWN_IDS]
FULL_MAX_SAMPLE_PER_TOWN = {"town" + t: 1e9 for t in _TOWN_IDS}                       # CFG:33

DATA = dict(
    pred_len=4,                                                                       # CFG:43
    is_local=True, is_full=False,                                                     # CFG:67-68
    history_query_index_lis=[-1, 0],                                                  # CFG:99
    camera_names=["rgb_front", "rgb_left", "rgb_right", "rgb_back"],                  # CFG:102
    seg_label_idxs=[1, 4, 5, 6, 7, 8, 10, 12, 18],                                    # CFG:108
)
TOTAL_EPOCHS = 60                                                                     # CFG:71
BATCH_SIZE_PER_GPU = 8                                                                # CFG:80
CKPT_INTERVAL = 1                                                                     # CFG:79
EVAL_INTERVAL = 1                                                                     # CFG:296


def data_config(dev=False, full=False):
    """The dataset cfg the reference assembles at CFG:81-95: `dev` is its is_dev branch (one town, 10 samples), `full` its
    is_full branch; else the TCP split.  -> dict with train_town, val_town, max_sample_per_town and the DATA fields."""
    c = copy.deepcopy(DATA)
    c["is_dev"], c["is_full"] = bool(dev), bool(full)
    if dev:
        c["train_town"], c["val_town"], c["max_sample_per_town"] = list(DEV_TRAIN), list(DEV_VAL), dict(DEV_MAX_SAMPLE_PER_TOWN)
    elif full:
        c["train_town"], c["val_town"], c["max_sample_per_town"] = list(FULL_TRAIN), list(FULL_VAL), dict(FULL_MAX_SAMPLE_PER_TOWN)
    else:
        c["train_town"], c["val_town"], c["max_sample_per_town"] = list(TCP_TRAIN), list(TCP_VAL), dict(TCP_MAX_SAMPLE_PER_TOWN)
    return c


def ida_aug_conf(final_dim=None):
    """calib.IDA_AUG_CONF (CFG:111-119), with `final_dim` and the resize limits scaled to a reduced image size."""
    c = dict(calib.IDA_AUG_CONF)
    if final_dim is not None and tuple(final_dim) != tuple(c["final_dim"]):
        base = c["final_dim"][0]
        c["final_dim"] = tuple(final_dim)
        c["resize_lim"] = tuple(r * final_dim[0] / base for r in c["resize_lim"])
    return c
