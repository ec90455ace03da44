"""The plan of an in-place Merkle update restated in Python (helper, no tests): which nodes a set of changed leaves dirties, where the one-workgroup
climb starts, which kernel a layer takes, and when the whole tree is rebuilt instead.  Worked out from the statement of the feature, as launch_plan
in test_gpu_merkle_plan.py is from the build's, not read off the device or the C++ header:

  * the pairs (index, leaf) apply in order, so of a repeated index the last pair counts; the leaf kernel gets the sorted unique indices;
  * a tree of 2^(sub_bits + cap_height) leaves is 2^cap_height cap subtrees; node g of layer l = 1 .. sub_bits, counted over all subtrees, is dirty
    when a changed leaf lies below it: g = leaf >> l;
  * the climb layer is the first layer with at most 64 dirty nodes (the counts never grow upwards); sub_bits + 1 when there is none;
  * Poseidon: the climb kernel takes the climb layer and every layer above it in one launch; below it a layer with at most 2^lanes_log dirty nodes
    takes the 16-lane kernel, a wider one the one-lane kernel.  BN254 has no 16-lane form: every layer takes its one-lane kernel;
  * an update of at least n_leaves >> full_log unique leaves writes the leaves and rebuilds every level with the build's own launch plan."""
import numpy as np

from test_gpu_merkle_plan import launch_plan

CLIMB_MAX = 64
POSEIDON, BN254 = 0, 1
OPT_MERKLE_LANES_LOG, OPT_MERKLE_UPDATE_FULL_LOG = 1, 8
LANES_LOG_DEFAULT, FULL_LOG_DEFAULT = 14, 4      # include/gl355.h; the second from the crossover in profiles/merkle_update.txt


def dedup(indices):
    """-> (sorted unique leaves, position of each one's last occurrence)"""
    last = {}
    for pos, i in enumerate(indices):
        last[int(i)] = pos
    leaves = sorted(last)
    return leaves, [last[i] for i in leaves]


def dirty_layers(leaves, sub_bits):
    """{layer: sorted unique dirty node ids}, layers 1 .. sub_bits"""
    return {layer: sorted({i >> layer for i in leaves}) for layer in range(1, sub_bits + 1)}


def climb_layer(dirty, sub_bits):
    for layer in range(1, sub_bits + 1):
        if len(dirty[layer]) <= CLIMB_MAX:
            return layer
    return sub_bits + 1


def is_full(n_unique, n_leaves, full_log):
    return n_unique >= (n_leaves >> full_log)


def kernel_of(dirty, climb, layer, lanes_log, lanes16=True):
    if not lanes16:
        return "level"
    if layer >= climb:
        return "climb"
    return "lanes" if len(dirty[layer]) <= (1 << lanes_log) else "level"


def plan_line(sub_bits, cap_height, lanes_log, lanes16, full_log, indices):
    """what tests/merkle_update_plan_check.cpp answers"""
    leaves, src = dedup(indices)
    dirty = dirty_layers(leaves, sub_bits)
    climb = climb_layer(dirty, sub_bits)
    widest = max([len(leaves)] + [len(d) for d in dirty.values()])
    s = "leaves=%s src=%s climb=%d full=%d fit=%d " % (",".join(map(str, leaves)), ",".join(map(str, src)), climb,
                                                      is_full(len(leaves), 1 << (sub_bits + cap_height), full_log), (widest + 3) // 4 <= 0x7FFFFFFF)
    return s + "".join("|%d:%s:%s" % (layer, kernel_of(dirty, climb, layer, lanes_log, lanes16), ",".join(map(str, dirty[layer])))
                       for layer in range(1, sub_bits + 1))


def kernel_mix(log_n, cap_height, indices, lanes_log=LANES_LOG_DEFAULT, full_log=FULL_LOG_DEFAULT, hasher=POSEIDON):
    """{profile scope: launches} of one update"""
    sub_bits = log_n - cap_height
    leaves, _ = dedup(indices)
    pre = "bn254_" if hasher == BN254 else ""
    mix = {pre + "merkle_update_leaves_kernel": 1 if leaves else 0}
    if not leaves:
        return mix
    if is_full(len(leaves), 1 << log_n, full_log):
        if hasher == BN254:      # bn254_above_leaves: every level one launch, 32 lanes per node below 2^13 nodes
            n_lanes = sum(1 for layer in range(1, sub_bits + 1) if (1 << log_n) >> layer <= (1 << 13) - 1)
            mix.update({"bn254_merkle_level_lanes_kernel": n_lanes, "bn254_merkle_level_kernel": sub_bits - n_lanes})
        else:
            level, lanes, top = launch_plan(log_n, cap_height, lanes_log)
            mix.update({"merkle_level_kernel": level, "merkle_level_lanes_kernel": lanes, "merkle_top_kernel": 1 if top else 0})
        return {k: v for k, v in mix.items() if v}
    dirty = dirty_layers(leaves, sub_bits)
    climb = climb_layer(dirty, sub_bits)
    names = {"level": pre + "merkle_update_level_kernel", "lanes": "merkle_update_level_lanes_kernel", "climb": "merkle_update_climb_kernel"}
    for layer in range(1, sub_bits + 1):
        which = kernel_of(dirty, climb, layer, lanes_log, hasher == POSEIDON)
        mix[names[which]] = mix.get(names[which], 0) + 1
        if which == "climb":
            break
    return mix


UPDATE_SCOPES = ("merkle_update_leaves_kernel", "merkle_update_level_kernel", "merkle_update_level_lanes_kernel", "merkle_update_climb_kernel",
                 "merkle_level_kernel", "merkle_level_lanes_kernel", "merkle_top_kernel", "bn254_merkle_update_leaves_kernel",
                 "bn254_merkle_update_level_kernel", "bn254_merkle_level_kernel", "bn254_merkle_level_lanes_kernel")


def mix_of_profile(prof):
    return {k: prof[k][0] for k in UPDATE_SCOPES if k in prof and prof[k][0]}


def apply_updates(leaves, updates):
    """the leaf array after the (indices, rows) pairs of `updates`, each applied in order"""
    out = np.array(leaves, dtype=np.uint64, copy=True)
    for indices, rows in updates:
        for i, row in zip(indices, rows):
            out[int(i)] = row
    return out


def expected(orc, leaves, updates, cap_height):
    """(leaves, digests, cap) of the CPU oracle's merkle_build on the updated array -- the reference for every byte; orc: the session's Oracle, or
    its Bn254Oracle for the second hasher"""
    lv = apply_updates(leaves, updates)
    dig, cap = orc.merkle_build(lv, cap_height)
    return lv, dig, cap
