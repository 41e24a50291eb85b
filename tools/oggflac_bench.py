#!/usr/bin/env python3
"""Ogg FLAC on the GPU: batch decode of device-resident .oga images, timed per
stage with HIP events (atg_decoder_kernel_times), against the native FLAC
decode of the same frames in the same process, and against the reference's
standalone decoder where oracle/_ref/oggflacdec exists.

Default shape: 1024 tracks x 10 s of `tone` (tests/signals.py) at 44.1 kHz,
16-bit stereo, FLAC-8 frames from the GPU encoder, muxed two ways with
tests/oggflac_port.py: one packet per page (libFLAC's habit) and 255-segment
pages.  The tracks are `--distinct` different signals repeated over the batch.
The Ogg decodes and the native decode alternate step by step; 2 warm-up and 20
timed steps each.  Every decoded track is verified: status 0, and the MD5 of
its PCM equal to the source's.

The container pass moves each image about three times (the checksum pass
reads it, the gather reads and writes it): that over 8 TB/s is the roofline
share given for its kernels.  Writes one JSON document (--out, default
profiles/oggflac_bench.json) and prints it.

--encode measures the other direction instead: the Ogg FLAC batch encode
(atg_oggflac_encode_device) of device-made PCM in both page layouts -- a page
per packet (the default) and filled 255-segment pages -- against the native
atg_flac_encode_device of the same batch, alternating step by step in one
process.  Every Ogg image is decoded back on the GPU (status 0, MD5 equal to
the source's) and 4 images are compared byte for byte with
tests/oggflac_mux_port.py.  The container phases (ogg_plan, ogg_pages,
ogg_split, ogg_crc of atg_engine_kernel_times) move the image about three
times: the split reads and writes it, the checksum pass reads it.  There is
no reference Ogg FLAC encoder (the reference calls the external `flac --ogg`);
where oracle/_ref/oggflacdec exists its decode of the same images at --procs
processes is recorded for scale only.  Default output:
profiles/oggflac_enc_bench.json.
"""
import argparse
import concurrent.futures
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "python-audio-tools_amd"), os.path.join(ROOT, "tests")]
REF_DEC = os.path.join(ROOT, "oracle", "_ref", "oggflacdec")
HBM_BYTES_PER_S = 8e12  # MI355X peak


def mean_times(rows):
    return {k: float(np.mean([r[k] for r in rows])) for k in rows[0]}


def spread(xs):
    return {"mean": float(np.mean(xs)), "min": float(np.min(xs)), "max": float(np.max(xs)),
            "std": float(np.std(xs))}


def reference_run(images, n_tracks, procs):
    with tempfile.TemporaryDirectory() as tmp:
        for k, img in enumerate(images):
            with open(os.path.join(tmp, "%d.oga" % k), "wb") as f:
                f.write(img)

        def one(k):
            subprocess.run([REF_DEC, os.path.join(tmp, "%d.oga" % (k % len(images)))],
                           stdout=subprocess.DEVNULL, check=True)

        t0 = time.perf_counter()
        with concurrent.futures.ThreadPoolExecutor(procs) as ex:
            list(ex.map(one, range(n_tracks)))
        return time.perf_counter() - t0


def encode_main(args):
    import torch
    import oggflac_mux_port as mp
    import oracle_port
    from audiotools import _atgpu

    ch, bps, rate = 2, 16, args.rate
    n = int(args.seconds * rate)
    distinct = min(args.distinct, args.tracks)
    torch.cuda.init()
    # the PCM, made on the device: two sines per channel and noise
    g = torch.Generator(device="cuda").manual_seed(1)
    t = torch.arange(n, device="cuda", dtype=torch.float64)[:, None]
    sig = []
    for k in range(distinct):
        f = torch.rand(2, ch, device="cuda", generator=g, dtype=torch.float64)
        x = (0.35 * torch.sin(2 * np.pi * (100 + 1900 * f[0]) * t / rate) +
             0.25 * torch.sin(2 * np.pi * (2000 + 10000 * f[1]) * t / rate)) * 32767
        x = x + 8.0 * torch.randn(n, ch, device="cuda", generator=g, dtype=torch.float64)
        sig.append(x.round().clamp(-32768, 32767).to(torch.int16))
    src = [x.cpu().numpy().reshape(-1) for x in sig]
    want_md5 = [hashlib.md5(x.astype("<i2").tobytes()).digest() for x in src]
    pcm = torch.stack([sig[k % distinct] for k in range(args.tracks)]).contiguous()
    del sig
    tracks = _atgpu.TrackTable([(k * n, n) for k in range(args.tracks)])
    preset = dict(oracle_port.PRESETS["8"])
    opts = _atgpu.make_options(**preset)
    eng = _atgpu.Engine(0)
    serial = 0x4F676721
    layouts = {"page_per_packet": dict(page_segments=255, page_per_packet=True),
               "filled_255": dict(page_segments=255, page_per_packet=False)}
    ogg = {k: _atgpu.oggflac_enc_options(serial, **v) for k, v in layouts.items()}
    plain = [(k * n, n) for k in range(args.tracks)]
    nf, cap = eng.bounds(opts, plain, ch, bps)
    for o in ogg.values():
        cap = max(cap, eng.oggflac_bounds(opts, o, plain, ch, bps)[1])
    out = torch.empty(cap + 64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    names = list(layouts) + ["native"]
    rows, walls, last = {k: [] for k in names}, {k: [] for k in names}, {}
    for step in range(args.warmup + args.steps):
        for name in names:
            t0 = time.perf_counter()
            if name == "native":
                r = eng.encode_device(opts, pcm.data_ptr(), _atgpu.PCM_S16, tracks, ch, bps, rate,
                                      out.data_ptr(), cap)
            else:
                r, _, _ = eng.encode_oggflac_device(opts, ogg[name], pcm.data_ptr(),
                                                    _atgpu.PCM_S16, tracks, ch, bps, rate,
                                                    out.data_ptr(), cap)
            wall = (time.perf_counter() - t0) * 1e3
            if step >= args.warmup:
                rows[name].append(eng.kernel_times())
                walls[name].append(wall)
    # verify: every image of both layouts decoded back on the GPU, 4 compared
    # with the port; the reference's decoder on them for scale
    dec = _atgpu.Decoder(0)
    bad, compared, ref_s, image_bytes, pages = {}, {}, {}, {}, {}
    for name in layouts:
        r, _, _ = eng.encode_oggflac_device(opts, ogg[name], pcm.data_ptr(), _atgpu.PCM_S16,
                                            tracks, ch, bps, rate, out.data_ptr(), cap)
        image_bytes[name] = int(sum(x.bytes for x in r))
        pages[name] = int(sum(x.pages for x in r))
        dr, _, _ = dec.decode_oggflac_device(
            out.data_ptr(), cap, [_atgpu.oggflac_dec_track(x.out_offset, x.bytes) for x in r])
        bad[name] = int(sum(not (d.status == 0 and d.ogg_status == 0 and d.pcm_frames == n and
                                 bytes(d.md5) == want_md5[k % distinct] and
                                 bytes(x.md5) == want_md5[k % distinct])
                            for k, (d, x) in enumerate(zip(dr, r))))
        picks = sorted(set([0, 1, args.tracks // 2, args.tracks - 1]))
        same, images = 0, []
        for k in picks:
            img = out[r[k].out_offset:r[k].out_offset + r[k].bytes].cpu().numpy().tobytes()
            want = mp.encode(src[k % distinct], ch, bps, rate,
                             dict(layouts[name], serial_number=serial + k), **preset)["image"]
            same += img == want
            images.append(img)
        compared[name] = {"tracks": picks, "equal_to_port": int(same)}
        if os.path.exists(REF_DEC) and not args.no_reference:
            ref_s[name] = reference_run(images, args.tracks, args.procs)
    dec.close()
    eng.close()

    native = mean_times(rows["native"])
    native_wall = float(np.mean(walls["native"]))
    doc = {"shape": {"tracks": args.tracks, "seconds": args.seconds, "rate": rate, "channels": ch,
                     "bits_per_sample": bps, "kind": "two sines + noise, made on the device",
                     "distinct_signals": distinct, "flac_frames": nf, "warmup": args.warmup,
                     "steps": args.steps, "device": torch.cuda.get_device_name(0)},
           "verify": {"tracks": args.tracks, "tracks_not_verified": bad,
                      "compared_with_port": compared},
           "native_flac": {"stage_ms": native, "wall_ms_per_batch": spread(walls["native"])}}
    for name in layouts:
        ms = mean_times(rows[name])
        wall = float(np.mean(walls[name]))
        phases = {k: ms[k] for k in ("ogg_plan", "ogg_pages", "ogg_split", "ogg_crc")}
        container = sum(phases.values())
        moved = 3 * image_bytes[name]
        diff = wall - native_wall
        doc[name] = {
            "stage_ms": ms, "wall_ms_per_batch": spread(walls[name]),
            "over_native_wall": wall / native_wall, "wall_minus_native_ms": diff,
            "container_ms": container, "container_phases_ms": phases,
            "largest_container_phase": max(phases, key=phases.get),
            "host_side_of_the_difference_ms": diff - container,
            "image_bytes": image_bytes[name], "pages": pages[name],
            "container_bytes_moved": moved,
            "container_fraction_of_8TBps": moved / (container * 1e-3) / HBM_BYTES_PER_S,
            "pcm_frames_per_s_wall": n * args.tracks / (wall * 1e-3)}
        if name in ref_s:
            doc[name]["reference_decoder_s"] = ref_s[name]
    doc["reference"] = (
        "no reference Ogg FLAC encoder exists (the reference pipes PCM to the external "
        "`flac --ogg`): nothing here is a baseline for the encode. " +
        ("reference_decoder_s is oracle/_ref/oggflacdec DECODING the same images, %d processes "
         "at a time, same host, for scale only" % args.procs if ref_s
         else "oracle/_ref/oggflacdec absent or skipped"))
    text = json.dumps(doc, indent=1, sort_keys=True)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    ok = not any(bad.values()) and all(c["equal_to_port"] == len(c["tracks"])
                                       for c in compared.values())
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--no-reference", action="store_true")
    ap.add_argument("--encode", action="store_true",
                    help="measure the Ogg FLAC encoder instead (see the module text)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "oggflac_enc_bench.json" if args.encode
                                else "oggflac_bench.json")
    if args.encode:
        return encode_main(args)

    import torch
    import oggflac_port as op
    import oracle_port
    import signals
    from audiotools import _atgpu

    ch, bps, rate = 2, 16, args.rate
    n = int(args.seconds * rate)
    distinct = min(args.distinct, args.tracks)
    torch.cuda.init()
    pcms = [signals.make("tone", n, ch, bps, seed=100 + k) for k in range(distinct)]
    want_md5 = [hashlib.md5(p.astype("<i2").tobytes()).digest() for p in pcms]
    # FLAC-8 frames from the GPU encoder
    eng = _atgpu.Engine(0)
    out, res, _, _ = eng.encode(_atgpu.make_options(**oracle_port.PRESETS["8"]),
                                np.concatenate(pcms).astype(np.int16),
                                [(k * n, n) for k in range(distinct)], ch, bps, rate)
    flacs = [out[r.out_offset:r.out_offset + r.bytes].tobytes() for r in res]
    eng.close()
    layouts = {"packet_per_page": [], "pages_of_255": []}
    bodies, infos = [], []
    for img in flacs:
        pk, nh = op.flac_packets(img)
        # a page per packet: the segments of each packet on a page of its own
        pages, seq = [], 0
        for i, p in enumerate(pk):
            lv = op.lacing_of(len(p))
            for a in range(0, len(lv), 255):
                flags = (1 if a else 0) | (2 if seq == 0 else 0) | \
                    (4 if i == len(pk) - 1 and a + 255 >= len(lv) else 0)
                pages.append(op.page(lv[a:a + 255], p[255 * a:255 * a + sum(lv[a:a + 255])],
                                     flags, granule=seq, sequence=seq))
                seq += 1
        layouts["packet_per_page"].append(b"".join(pages))
        layouts["pages_of_255"].append(op.mux(pk, segs_per_page=255))
        rc, si, _ = _atgpu.read_metadata(img)
        assert rc == 0
        infos.append(si)
        bodies.append(img[si.frames_offset:])
    n_frames = len(pk) - 1 - nh

    def batch(images):
        data, tracks = _atgpu.oggflac_pack([images[k % distinct] for k in range(args.tracks)])
        buf = torch.frombuffer(bytearray(data + bytes(64)), dtype=torch.uint8).cuda()
        return buf, len(data), tracks

    dev = {name: batch(imgs) for name, imgs in layouts.items()}
    parts, ntracks, pos = [], [], 0
    for k in range(args.tracks):
        body = bodies[k % distinct]
        ntracks.append(_atgpu.dec_track(pos, len(body), infos[k % distinct]))
        parts.append(body + bytes((-len(body)) % 4))
        pos += len(parts[-1])
    nbuf = torch.frombuffer(bytearray(b"".join(parts) + bytes(64)), dtype=torch.uint8).cuda()
    del parts
    torch.cuda.synchronize()

    dec = _atgpu.Decoder(0)
    rows = {k: [] for k in list(dev) + ["native"]}
    walls = {k: [] for k in rows}
    bad = {k: 0 for k in rows}
    last = {}
    for step in range(args.warmup + args.steps):
        for name in rows:
            t0 = time.perf_counter()
            if name == "native":
                r, _, _ = dec.decode_device(nbuf.data_ptr(), pos, ntracks)
            else:
                buf, nbytes, tracks = dev[name]
                r, _, _ = dec.decode_oggflac_device(buf.data_ptr(), nbytes, tracks)
            wall = (time.perf_counter() - t0) * 1e3
            last[name] = r
            if step >= args.warmup:
                rows[name].append(dec.kernel_times())
                walls[name].append(wall)
    for name, r in last.items():
        for k, x in enumerate(r):
            ok = x.status == 0 and bytes(x.md5) == want_md5[k % distinct] and x.pcm_frames == n
            if name != "native":
                ok = ok and x.ogg_status == 0
            bad[name] += not ok
    dec.close()

    ref_s = None
    if os.path.exists(REF_DEC) and not args.no_reference:
        ref_s = {name: reference_run(imgs, args.tracks, args.procs)
                 for name, imgs in layouts.items()}

    doc = {"shape": {"tracks": args.tracks, "seconds": args.seconds, "rate": rate, "channels": ch,
                     "bits_per_sample": bps, "kind": "tone", "distinct_signals": distinct,
                     "flac_frames_per_track": n_frames, "warmup": args.warmup,
                     "steps": args.steps, "device": torch.cuda.get_device_name(0)},
           "verify": {"tracks": args.tracks, "tracks_not_verified": bad},
           "native_flac": {"stage_ms": mean_times(rows["native"]),
                           "wall_ms_per_batch": spread(walls["native"]),
                           "batch_bytes": pos}}
    native_total = doc["native_flac"]["stage_ms"]["dec_total"]
    for name in layouts:
        ms = mean_times(rows[name])
        nbytes = dev[name][1]
        demux = ms["ogg_walk"] + ms["ogg_crc"] + ms["ogg_gather"]
        moved = 3 * nbytes
        d = {"stage_ms": ms, "wall_ms_per_batch": spread(walls[name]), "batch_bytes": nbytes,
             "pages": int(sum(x.pages for x in last[name])),
             "packets": int(sum(x.packets for x in last[name])),
             "demux_ms": demux, "flac_part_ms": ms["dec_total"],
             "flac_part_over_native": ms["dec_total"] / native_total,
             "demux_bytes_moved": moved,
             "demux_fraction_of_8TBps": moved / (demux * 1e-3) / HBM_BYTES_PER_S,
             "pcm_frames_per_s_wall": n * args.tracks / (float(np.mean(walls[name])) * 1e-3)}
        if ref_s:
            d["reference_s"] = ref_s[name]
            d["speedup_over_reference_wall"] = ref_s[name] / (float(np.mean(walls[name])) * 1e-3)
        doc[name] = d
    doc["reference"] = ("oracle/_ref/oggflacdec, %d processes at a time, same host" % args.procs
                        if ref_s else "skipped: oracle/_ref/oggflacdec absent")
    text = json.dumps(doc, indent=1, sort_keys=True)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 1 if any(bad.values()) else 0


if __name__ == "__main__":
    sys.exit(main())
