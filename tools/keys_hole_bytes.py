"""The bytes K2's descriptor stream reads for the first pairs of a synthetic population, and the share its key and
shape holes leave out (gpudiff_pair_stream_bytes, include/gpudiff_format.h), summed on the host from the product
encoder's rows: both sums, with the key holes alone (gpudiff_rows_stream_bytes, DESIGN.md §6n's measure) and with the
shape holes the kernel honours (gpudiff_rows_read_bytes), and what it reads when every pair that can be is streamed from
the batch's compare image (gpudiff_rows_image_read_bytes, the slots' sum), with and without the status shape bit, and
with the imaged pairs' parts packed to their values' true lengths (gpudiff_rows_image_streamed_bytes: what K2 really
streams).  No GPU needed.

    python tools/keys_hole_bytes.py --config config3 --population 200000 --pairs 100000
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="config3")
    ap.add_argument("--population", type=int, default=200000, help="pairs of the population (clusters: a hundredth)")
    ap.add_argument("--pairs", type=int, default=100000, help="its first pairs, encoded and summed")
    ap.add_argument("--threads", type=int, default=8)
    args = ap.parse_args()
    from kcp_amd import gpudiff as G
    from kcp_amd import synth as S

    pop = S.Population(S.make_cfg(args.config, n_pairs=args.population, n_clusters=max(1, args.population // 100)))
    eng = G.Engine(device=G.DEVICE_NONE, encode_threads=args.threads)
    n = min(args.pairs, pop.n)
    out = dict(config=args.config, pairs=n, format_bytes=0, stream_bytes=0, read_bytes=0, stream_bytes_no_holes=0,
               sizes_eq=0, keys_eq=0, shape_eq=0, pairs_with_hole=0, pairs_with_shape_hole=0, image_read_bytes=0,
               image_read_bytes_spec_only=0, imaged=0, imaged_stat_sized=0, imaged_stat_shape_eq=0,
               image_slot_bytes_imaged=0, image_streamed_bytes=0)
    pos = 0
    while pos < n:
        m = min(65536, n - pos)
        hb = pop.chunk(eng, pos, m, args.threads).hb
        rows = hb.rows()
        ok = ((rows["flags_a"] | rows["flags_b"]) & G.OBJ_DECODE_ERR) == 0
        eq = ok & (rows["spec_l_a"] == rows["spec_l_b"]) & (rows["spec_ar_a"] == rows["spec_ar_b"])
        bit = (rows["flags_b"] & G.OBJ_SPEC_KEYS_EQ) != 0
        sbit = bit & ((rows["flags_b"] & G.OBJ_SPEC_SHAPE_EQ) != 0)
        L = rows["spec_l_a"].astype(np.int64)
        hole = (12 * L // 128 * 128) > ((8 * L + 127) // 128 * 128)
        shole = (16 * L // 128 * 128) > ((8 * L + 127) // 128 * 128)
        out["format_bytes"] += int(G.cluster_bytes(rows, int(rows["cluster_id"].max()) + 1).sum())
        out["stream_bytes"] += G.stream_bytes(rows)
        out["read_bytes"] += G.read_bytes(rows)
        plain = rows.copy()
        plain["flags_b"] &= ~np.uint32(G.OBJ_SPEC_KEYS_EQ)
        out["stream_bytes_no_holes"] += G.stream_bytes(plain)
        out["sizes_eq"] += int(eq.sum())
        out["keys_eq"] += int((eq & bit).sum())
        out["shape_eq"] += int((eq & sbit).sum())
        out["pairs_with_hole"] += int((eq & bit & hole).sum())
        out["pairs_with_shape_hole"] += int((eq & sbit & shole).sum())
        # the compare image: every spec-shape-equal pair is imaged; its status part is compacted under the status bit
        out["image_read_bytes"] += G.image_read_bytes(rows)
        nostat = rows.copy()
        nostat["flags_b"] &= ~np.uint32(G.OBJ_STAT_SHAPE_EQ)
        out["image_read_bytes_spec_only"] += G.image_read_bytes(nostat)
        # ... and its parts are packed to the values' true lengths: what K2 streams of the imaged pairs, beside what
        # their slots would give (image_read_bytes is the slots' sum, an upper bound)
        out["image_slot_bytes_imaged"] += G.image_read_bytes(rows[eq & sbit])
        out["image_streamed_bytes"] += G.image_streamed_bytes(rows, hb.pool_view())
        stat_sz = ((rows["flags_b"] & G.OBJ_HAS_STATUS) != 0) & (rows["stat_l_a"] == rows["stat_l_b"]) & (
            rows["stat_ar_a"] == rows["stat_ar_b"])
        out["imaged"] += int((eq & sbit).sum())
        out["imaged_stat_sized"] += int((eq & sbit & stat_sz).sum())
        out["imaged_stat_shape_eq"] += int((eq & sbit & stat_sz & ((rows["flags_b"] & G.OBJ_STAT_SHAPE_EQ) != 0)).sum())
        hb.free()
        pos += m
    out["hole_bytes"] = out["stream_bytes_no_holes"] - out["stream_bytes"]
    out["hole_bytes_per_pair"] = out["hole_bytes"] / n
    out["stream_bytes_per_pair_no_holes"] = out["stream_bytes_no_holes"] / n
    out["hole_share"] = out["hole_bytes"] / out["stream_bytes_no_holes"]
    out["shape_hole_bytes"] = out["stream_bytes_no_holes"] - out["read_bytes"]
    out["shape_hole_bytes_per_pair"] = out["shape_hole_bytes"] / n
    out["shape_hole_share"] = out["shape_hole_bytes"] / out["stream_bytes_no_holes"]
    out["read_over_stream"] = out["read_bytes"] / out["stream_bytes"]
    out["read_bytes_per_pair"] = out["read_bytes"] / n
    out["image_saved_bytes_per_pair"] = (out["read_bytes"] - out["image_read_bytes"]) / n
    out["image_saved_share"] = (out["read_bytes"] - out["image_read_bytes"]) / out["read_bytes"]
    out["image_saved_bytes_per_pair_spec_only"] = (out["read_bytes"] - out["image_read_bytes_spec_only"]) / n
    out["image_saved_share_spec_only"] = (out["read_bytes"] - out["image_read_bytes_spec_only"]) / out["read_bytes"]
    out["packed_read_bytes"] = out["image_read_bytes"] - out["image_slot_bytes_imaged"] + out["image_streamed_bytes"]
    out["packed_read_bytes_per_pair"] = out["packed_read_bytes"] / n
    out["packed_saved_bytes_per_pair"] = (out["image_read_bytes"] - out["packed_read_bytes"]) / n
    out["packed_saved_share"] = (out["image_read_bytes"] - out["packed_read_bytes"]) / out["image_read_bytes"]
    print(json.dumps(out))
    eng.close()
    pop.close()


if __name__ == "__main__":
    main()
