#!/usr/bin/env python3
"""The detection (AVA) input step of one batch: `gpu_detection_batch` (one table upload + one `sf_clip_batch_det`
launch) at the AVA shape, beside its bound and beside the reference's host preprocessing.

Shape: 8 clips, each its own span of 32 BGR frames of 256 x 340 uint8 (what `retry_load_images` yields), train split
with jitter [256, 320] and crop 224, PCA lighting on, alpha 4 (8 Slow frames), stem padding (3, 3); 10 boxes per clip.
  device   the kernel alone between two HIP events (table already uploaded), and the whole `gpu_detection_batch` call
           on the host clock between two device synchronisations (decisions excluded: they are drawn beforehand)
  bound    bytes the launch must move over HBM at 8 TB/s (MI355X peak): both output buffers written once, and the
           part of every source frame that the crop window covers read once
  host     (--host; needs the reference's tree, so the build container only, no GPU) the reference's own
           `Ava._images_and_boxes_preprocessing` + `pack_pathway_output` per clip and `detection_collate` for the batch
Also printed: the host-to-device bytes of each route (uint8 spans + the table against the float [slow, fast] tensors).
Method: warm-up, then ROUNDS rounds of REPS calls; the figure is the median round, the spread its min .. max.  Clocks
not pinned.  usage: tools/microbench/det_input_bench.py [--host] [out.txt]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "efficient-slowfast_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

B, T, H, W, CROP, ALPHA, PAD, KBOX = 8, 32, 256, 340, 224, 4, (3, 3), 10
ROUNDS, REPS = 9, 5
HBM_BYTES_PER_S = 8.0e12
MEAN, STD = [0.45, 0.45, 0.45], [0.225, 0.225, 0.225]


def ava_cfg():
    from slowfast.config.defaults import get_cfg
    cfg = get_cfg()
    cfg.AVA.IMG_PROC_BACKEND, cfg.AVA.TRAIN_USE_COLOR_AUGMENTATION = "pytorch", True
    cfg.DATA.NUM_FRAMES, cfg.DATA.TRAIN_JITTER_SCALES, cfg.DATA.TRAIN_CROP_SIZE = T, [256, 320], CROP
    cfg.DATA.MEAN, cfg.DATA.STD, cfg.SLOWFAST.ALPHA = MEAN, STD, ALPHA
    return cfg


def clips_and_boxes():
    rs = np.random.RandomState(1)
    clips = [rs.randint(0, 256, (T, H, W, 3)).astype(np.uint8) for _ in range(B)]
    xy = rs.uniform(0.0, 0.6, (B, KBOX, 2))
    boxes = np.concatenate([xy, xy + rs.uniform(0.05, 0.4, (B, KBOX, 2))], axis=2).clip(0, 1)
    return clips, boxes


def spread(ts, unit=1e6):
    return "%9.1f (%8.1f .. %8.1f)" % (statistics.median(ts) * unit, min(ts) * unit, max(ts) * unit)


def device_lines():
    import sfhip
    from slowfast.datasets import utils as ds
    assert torch.cuda.is_available(), "det_input_bench.py measures on an MI355X: no GPU, no figure"
    cfg = ava_cfg()
    clips, boxes01 = clips_and_boxes()
    videos = [torch.from_numpy(c).cuda() for c in clips]
    np.random.seed(1)
    params = [ds.det_clip_params(cfg, "train", H, W) for _ in range(B)]
    samples = [(torch.arange(T), p) for p in params]
    boxes = [ds.det_boxes(b, H, W, p) for b, p in zip(boxes01, params)]

    def whole():
        return ds.gpu_detection_batch(videos, samples, boxes, MEAN, STD, ALPHA, reverse_input_channel=True, pad=PAD)

    (slow, fast), bboxes = whole()
    slow_idx = ds.slow_frame_indices(T, ALPHA)
    table_host = ds.det_table(videos, samples, slow_idx)
    table = table_host.cuda()
    f2, s2 = torch.empty_like(fast.buf), torch.empty_like(slow.buf)

    def kernel():
        sfhip.clip_batch_det(table_host, table, slow_idx.numel(), (CROP, CROP), MEAN, STD, f2, s2, reverse=True,
                             ph=PAD[0], pw=PAD[1])

    kernel()
    torch.cuda.synchronize()
    same = torch.equal(f2.view(torch.int32), fast.buf.view(torch.int32)) and torch.equal(
        s2.view(torch.int32), slow.buf.view(torch.int32))
    t_kernel, t_whole = [], []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            kernel()
        e1.record()
        torch.cuda.synchronize()
        t_kernel.append(e0.elapsed_time(e1) * 1e-3 / REPS)
        t0 = time.perf_counter()
        for _ in range(REPS):
            whole()
        torch.cuda.synchronize()
        t_whole.append((time.perf_counter() - t0) / REPS)
    written = (fast.buf.numel() + slow.buf.numel()) * 4
    # the crop window's footprint in the source frame: CROP / new_h of its height, CROP / new_w of its width
    read = sum(T * 3 * (CROP * H / p.new_h) * (CROP * W / p.new_w) for p in params)
    bound = (written + read) / HBM_BYTES_PER_S
    up_device = sum(c.nbytes for c in clips) + (table_host.numel() + (5 * bboxes.shape[0] + 1) // 2) * 8
    up_host = B * 3 * (T + T // ALPHA) * CROP * CROP * 4 + bboxes.numel() * 4
    return [
        "AVA shape: %d clips of %d x %d x %d BGR uint8, train, jitter [256, 320], crop %d, PCA lighting, alpha %d, pad %s, "
        "%d boxes; direct launch and gpu_detection_batch bitwise equal: %s; median of %d rounds of %d calls (min .. max)" % (
            B, T, H, W, CROP, ALPHA, PAD, bboxes.shape[0], same, ROUNDS, REPS),
        "bytes over HBM: %.1f MB written + %.1f MB read (crop footprint) = %.1f MB; bound at 8 TB/s %9.1f us" % (
            written / 1e6, read / 1e6, (written + read) / 1e6, bound * 1e6),
        "sf_clip_batch_det, HIP events      %s us" % spread(t_kernel),
        "gpu_detection_batch, host clock    %s us  (table build, one upload, one launch)" % spread(t_whole),
        "host-to-device bytes: this route %.1f MB (uint8 spans + the table with the boxes), the reference's route %.1f MB "
        "(float [slow, fast] + boxes)" % (up_device / 1e6, up_host / 1e6),
    ]


def host_lines():
    sys.path[:0] = [os.path.join(ROOT, "tests", "golden")]
    import make_golden_detection_input as gen
    ava_dataset, transform, utils = gen.load_reference()
    loader = gen.load_reference_loader()
    clips, boxes01 = clips_and_boxes()
    case = dict(split="train", bgr=False, crop=CROP, jitter=[256, 320], color=True)
    dset = gen.make_dataset(ava_dataset, case)
    dset._data_mean, dset._data_std = MEAN, STD
    from make_golden_input import cfg_like
    pcfg = cfg_like(ALPHA, False)

    def batch():
        items = []
        for i, (c, b) in enumerate(zip(clips, boxes01)):
            imgs = torch.as_tensor(c).permute(0, 3, 1, 2)
            imgs, bx = dset._images_and_boxes_preprocessing(imgs, boxes=b.copy())
            frames = utils.pack_pathway_output(pcfg, imgs.permute(1, 0, 2, 3))
            items.append((frames, np.zeros((KBOX, 80), np.int32), i,
                          {"boxes": bx, "ori_boxes": b, "metadata": [[i, 900]] * KBOX}))
        return loader.detection_collate(items)

    np.random.seed(1)
    batch()
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        batch()
        ts.append(time.perf_counter() - t0)
    return ["reference host preprocessing of the same batch (Ava._images_and_boxes_preprocessing + pack_pathway_output "
            "per clip, detection_collate), %d torch threads, median of 5 (min .. max): %s ms" % (
                torch.get_num_threads(), spread(ts, 1e3))]


def main():
    argv = [a for a in sys.argv[1:] if a != "--host"]
    lines = host_lines() if "--host" in sys.argv[1:] else device_lines()
    text = "\n".join(lines)
    print(text)
    if argv:
        with open(argv[0], "a" if "--host" in sys.argv[1:] else "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
