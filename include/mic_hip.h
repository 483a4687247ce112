/*
 * mic_hip.h -- C ABI of libmic_hip.so, the MI355X (gfx950) implementation of MIC's
 * parallel-strip encode/decode hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.  The
 * reference's Go package reaches it through cgo exactly as it reaches its own C codec
 * today (reference: ojph/mic_c.go:11-19); INTEGRATION.md shows the binding.
 *
 * Conventions (reference: ojph/mic_compress_c.h:26-38, ojph/mic_decompress_c.h:24-50,
 * ojph/mic_parallel.h:49-57):
 *   - the caller allocates every buffer; the library keeps no caller pointer after return;
 *   - 0 = success, negative = error class (MIC_ERR_*);
 *   - every entry point is thread-safe and may be called concurrently from any OS thread
 *     (reference: mic_parallel.h:47-48);
 *   - encoders take the caller's max_value: the Go API passes it
 *     (multiframecompress.go:15), the reference C derives it (mic_compress_c.c:774-775).
 *
 * There is no CPU fallback: every call fails with MIC_ERR_DEVICE when no gfx950 device
 * is usable.
 */
#ifndef MIC_HIP_H
#define MIC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes --------------------------------------------------------------- */
#define MIC_OK                   0
#define MIC_ERR_ARGS            -1   /* bad pointer / dimension (mic_compress_c.c:918) */
#define MIC_ERR_NOMEM           -2
#define MIC_ERR_USE_RLE         -3   /* Go ErrUseRLE, fseu16.go:36; C: mic_compress_c.c:852 */
#define MIC_ERR_CAPACITY        -5   /* output buffer too small (mic_compress_c.c:865) */
#define MIC_ERR_CORRUPT         -6   /* malformed stream (mic_decompress_c.c:1004-1063) */
#define MIC_ERR_DEVICE          -7   /* HIP runtime / no gfx950 device */
#define MIC_ERR_INTERNAL        -8
#define MIC_ERR_UNSUPPORTED     -9
#define MIC_ERR_INCOMPRESSIBLE -10   /* Go ErrIncompressible, fseu16.go:33; C: -4 / -10 */
#define MIC_ERR_IO             -11   /* a read or write callback of the MIC3 streaming calls returned non-zero */
#define MIC_ERR_MISMATCH       -12   /* decoded pixels differ from the reference pixels / from the expected CRC-32 (the verify calls) */

/* FSE flavour requested from an encoder: the entry of the reference's fallback chain
 * (multiframecompress.go:15-93).  2 -> CompressSingleFrame (2-state, then 1-state),
 * 4 -> CompressSingleFrame4State (4 -> 2 -> 1), 8 -> CompressSingleFrame8State. */
#define MIC_STATES_2 2
#define MIC_STATES_4 4
#define MIC_STATES_8 8

/* ---- library / device ------------------------------------------------------------- */
/* Selects the HIP device of the DEFAULT session, i.e. of every entry point below that takes host pointers (default 0).
 * Returns MIC_ERR_DEVICE when the device does not exist or is not gfx950.  A process that drives several GPUs -- the
 * reference's host is ONE process (goroutines, parallelstrips.go:77-93; re-entrancy: ojph/mic_parallel.h:47-48) -- creates
 * one session per device with mic_hip_session_create_on and uses the session entry points. */
int mic_hip_set_device(int device);
/* SEVERAL devices for the batch entry points below (mic_hip_compress_batch / _decompress_batch, mic_hip_pics_compress_batch /
 * _decompress_batch, mic_hip_mic2_compress / _decompress, mic_hip_mic2_compress_batch / _decompress_batch, mic_hip_wavelet_v2_compress_batch / _decompress_batch / _decompress_level_batch) and for the MIC3
 * calls mic_hip_wsi_compress / _compress_ex (bands of tile rows, see there), mic_hip_wsi_decompress_level and
 * mic_hip_wsi_decompress_region (tile rows; a region of two tile rows or more): a call's jobs are cut into one contiguous shard per listed device,
 * balanced by pixels -- the static assignment of the reference's fan-outs (parallelstrips.go:77-93, multiframecompress.go:186-209,
 * wsicompress.go:126-145) -- and the shards run side by side, each on a session of its device's pool with its own sub-batch
 * pipeline and transfer streams; results are written straight into the caller's buffers (no gather: the caller's memory is the
 * whole view).  This is how ONE host process -- the reference's host is one Go process -- gets past a single PCIe link: eight GPUs
 * are eight links.  devices[0] is also the device of every other host-pointer entry point; a device may be listed twice (two
 * shards on one GPU).  Waits for running calls; MIC_ERR_DEVICE when a device does not exist or is not gfx950.
 * mic_hip_get_devices: the current list (returns its length; at most cap entries are written). */
int mic_hip_set_devices(const int *devices, int n);
int mic_hip_get_devices(int *devices, int cap);
/* The cut those calls make, for callers that want to lay their work out to match it: n items of the given weights (pixels) into
 * `shards` contiguous shards -- item i belongs to shard k iff first[k] <= i < first[k + 1]; first has shards + 1 entries.
 * Needs no device. */
int mic_hip_shard_plan(const uint64_t *weights, int n, int shards, int *first);
/* The bands mic_hip_wsi_compress_ex cuts a slide into over `shards` devices (arguments as there: tile sizes 0 = 256, levels <= 0 =
 * automatic).  *k_out = K, the top level every band codes itself; band b is the rows row_first[b] .. row_first[b + 1] - 1 (row_first
 * has shards + 1 entries; a band may be empty).  Needs no device. */
int mic_hip_wsi_band_plan(int width, int height, int tile_w, int tile_h, int levels, int shards, int *k_out, int *row_first);
/* "gfx950 <n CUs> ..." style description of the active device; "" if none. */
const char *mic_hip_device_name(void);
const char *mic_hip_version(void);

/* ---- unit codec: one frame / strip / plane ----------------------------------------- */
/* Replaces CompressSingleFrame{,4State,8State} (multiframecompress.go:15,38,67) and
 * mic_compress_{two,four,eight}_state (ojph/mic_compress_c.h:26-38).
 * out_cap >= MIC_HIP_FRAME_BOUND(width*height) is always sufficient: a frame whose every pixel escapes codes two tokens per
 * pixel, FSE only gives up (ErrIncompressible) at two bytes per token, and the NCount header of a 65536-symbol alphabet is < 128 KiB. */
#define MIC_HIP_FRAME_BOUND(npx) (4 * (size_t)(npx) + 135168)
/* The ONE capacity contract of every encoder below: a container's bound is the sum of its units' MIC_HIP_FRAME_BOUND plus its
 * header and table.  (The reference C allocates 2*w*h + 4096 per unit, ojph/mic_compress_c.c:918, and its Go wrapper 4*len + 4096,
 * ojph/mic_c.go:170; an all-escape frame needs the 4 bytes per pixel.)  Real frames code far below it: a caller that knows its
 * data may pass less and handle MIC_ERR_CAPACITY. */
#define MIC_HIP_PICS_BOUND(width, height, num_strips) \
    (20 + 8 * (size_t)(num_strips) + 4 * (size_t)(width) * (size_t)(height) + 135168 * (size_t)(num_strips))
#define MIC_HIP_MIC2_BOUND(width, height, nframes) \
    (20 + (size_t)(nframes) * (8 + MIC_HIP_FRAME_BOUND((size_t)(width) * (size_t)(height))))
int mic_hip_compress_frame(const uint16_t *pixels, int width, int height,
                           uint16_t max_value, int nstates,
                           uint8_t *out, size_t out_cap, size_t *out_len);

/* Replaces DecompressSingleFrame (multiframecompress.go:97) and
 * mic_decompress_{two,four,eight}_state (ojph/mic_decompress_c.h:24-50): the FSE flavour
 * (1/2/4/8-state, rANS-8) is auto-detected as in FSEDecompressU16Auto (fse2state.go:102). */
int mic_hip_decompress_frame(const uint8_t *compressed, size_t compressed_len,
                             uint16_t *pixels_out, int width, int height);

/* ---- bare FSE stage -------------------------------------------------------------------- */
/* Replaces FSECompressU16 (fsecompressu16.go:19), FSECompressU16TwoState (fse2state.go:22),
 * ...FourState (fse4state.go:24), ...EightState (fse8state.go:31) and RANSCompressU16EightState
 * (rans8state.go:31): flavour = 1, 2, 4, 8 or 108 (rANS-8).  No fallback chain: the sentinels
 * MIC_ERR_USE_RLE / MIC_ERR_INCOMPRESSIBLE come back exactly where the Go functions return
 * ErrUseRLE / ErrIncompressible.  out_cap >= 2*n + 135168 is always sufficient (past two bytes per symbol the encoders
 * return MIC_ERR_INCOMPRESSIBLE; the NCount header of a 65536-symbol alphabet is < 128 KiB). */
int mic_hip_fse_compress_u16(const uint16_t *symbols, size_t n, int flavour,
                             uint8_t *out, size_t out_cap, size_t *out_len);
/* The same with the caller's ScratchU16.TableLog (fseu16.go:101-102): the value optimalTableLog starts from
 * (fsecompressu16.go:480-518; 0 = the default 11, > 16 = MIC_ERR_ARGS like prepare(), fseu16.go:136-138).
 * ScratchU16.MaxSymbolValue (fseu16.go:98-99) has no counterpart: the reference only defaults it, nothing reads it. */
int mic_hip_fse_compress_u16_ex(const uint16_t *symbols, size_t n, int flavour, int table_log,
                                uint8_t *out, size_t out_cap, size_t *out_len);
/* Replaces FSEDecompressU16Auto (fse2state.go:102-116): magic-byte dispatch over all five
 * flavours.  *out_n receives the number of symbols written. */
int mic_hip_fse_decompress_u16_auto(const uint8_t *in, size_t in_len,
                                    uint16_t *out, size_t out_cap, size_t *out_n);
/* The same with the caller's ScratchU16.DecompressLimit (fseu16.go:87-91; 0 = the default 2 GiB - 1): MIC_ERR_CAPACITY exactly
 * where the reference returns "output size > DecompressLimit" -- it compares at every wrap of its 65536-symbol ring (and, for
 * 1-state streams, at the end), so an N-state stream of `count` symbols fails iff floor(count / 65536) * 65536 >= limit. */
int mic_hip_fse_decompress_u16_ex(const uint8_t *in, size_t in_len, int64_t decompress_limit,
                                  uint16_t *out, size_t out_cap, size_t *out_n);

/* ---- batch: many independent units in one call (one cgo crossing, one launch chain) --- */
/* Replaces the goroutine fan-out of parallelstrips.go:77-93 / :292-321, the frame loop of
 * multiframecompress.go:186-209 and the tile worker pool of wsicompress.go:126-145. */
typedef struct mic_hip_enc_job {
    const uint16_t *pixels;   /* in : width*height u16, row-major (host memory) */
    int32_t   width, height;  /* in  */
    uint16_t  max_value;      /* in  */
    uint16_t  nstates;        /* in : MIC_STATES_2/4/8 */
    uint8_t  *out;            /* in : caller buffer */
    size_t    out_cap;        /* in  */
    size_t    out_len;        /* out */
    int32_t   status;         /* out: MIC_OK or MIC_ERR_* for this unit */
    int32_t   nstates_used;   /* out: 8/4/2/1 flavour actually written */
} mic_hip_enc_job;

typedef struct mic_hip_dec_job {
    const uint8_t *compressed; /* in  (host memory) */
    size_t    compressed_len;  /* in  */
    uint16_t *pixels_out;      /* in : width*height u16 (host memory) */
    int32_t   width, height;   /* in  */
    int32_t   status;          /* out */
} mic_hip_dec_job;

/* Return value: MIC_OK when the batch ran (inspect per-job status), or a global error.
 * Host buffers are ordinary (pageable) memory or pinned memory (below); large batches run as a pipeline of sub-batches --
 * upload, kernels and download of neighbouring sub-batches overlap -- and concurrent callers run on different sessions of a
 * small pool (MIC_HIP_POOL sessions, default 3), as the reference's C codec runs concurrent goroutines (ojph/mic_parallel.h:47-48).
 * Environment, read once: MIC_HIP_WS_BUDGET_MB (device memory a default session may grow to), MIC_HIP_PIPELINE_PARTS (force the
 * number of sub-batches), MIC_HIP_TRACE=1 (on stderr: every call's parts, the decode pipeline's stages with wall times, the devices' shards). */
int mic_hip_compress_batch(mic_hip_enc_job *jobs, int njobs);
int mic_hip_decompress_batch(mic_hip_dec_job *jobs, int njobs);

/* Pinned host memory (hipHostMalloc) for a caller's frame and stream buffers: every entry point that takes host pointers
 * recognises such memory -- and memory the caller registered itself -- and DMAs it in place; ordinary memory (a Go slice) is staged
 * through pinned slots by the library's transfer threads (MIC_HIP_IO_THREADS, default half the host's cores, at most 8).
 * A cgo caller wraps the pointer with unsafe.Slice. */
void *mic_hip_host_alloc(size_t bytes);
void  mic_hip_host_free(void *p);

/* ---- PICS container --------------------------------------------------------------------- */
/* Replaces CompressParallelStrips{,4State,8State} (parallelstrips.go:55,128,199).
 * num_strips <= 0 is rejected with MIC_ERR_ARGS: the Go default (GOMAXPROCS) is a host
 * property and stays on the Go side.  out_cap >= MIC_HIP_PICS_BOUND(width, height, num_strips) is always sufficient. */
int mic_hip_pics_compress(const uint16_t *pixels, int width, int height,
                          uint16_t max_value, int num_strips, int nstates,
                          uint8_t *out, size_t out_cap, size_t *out_len);
/* The same with the index of the strip the error belongs to (the reference wraps it: "parallelstrips: strip %d: %w",
 * parallelstrips.go:97): *failed_strip = the first strip whose codec failed, -1 when the call succeeded or the error is not a
 * strip's (arguments, capacity of the header, the device). */
int mic_hip_pics_compress_ex(const uint16_t *pixels, int width, int height,
                             uint16_t max_value, int num_strips, int nstates,
                             uint8_t *out, size_t out_cap, size_t *out_len, int *failed_strip);
/* Header probe (parallelstrips.go:271-286). */
int mic_hip_pics_info(const uint8_t *compressed, size_t compressed_len,
                      int *width, int *height, int *num_strips, int *strip_height);
/* Replaces DecompressParallelStrips (parallelstrips.go:270) and mic_decompress_parallel
 * (ojph/mic_parallel.h:49-52; max_threads has no meaning on the GPU and is dropped).
 * width/height must equal the header's. */
int mic_hip_pics_decompress(const uint8_t *compressed, size_t compressed_len,
                            uint16_t *pixels_out, int width, int height);
/* ... and with the index of the strip that failed to decode ("parallelstrips: strip %d: %w", parallelstrips.go:316; -1: none). */
int mic_hip_pics_decompress_ex(const uint8_t *compressed, size_t compressed_len,
                               uint16_t *pixels_out, int width, int height, int *failed_strip);
/* Many images, one call: the strips of ALL jobs are one unit batch (the reference reaches the same parallelism by calling
 * CompressParallelStrips from many goroutines, each fanning out its strips: parallelstrips.go:77-93; a single image is eight
 * serial entropy chains and leaves the device idle).  Every job's file equals mic_hip_pics_compress's, byte for byte. */
typedef struct mic_hip_pics_enc_job {
    const uint16_t *pixels;   /* in : width*height u16 (host memory) */
    int32_t   width, height;  /* in  */
    uint16_t  max_value;      /* in  */
    uint16_t  nstates;        /* in : MIC_STATES_2/4/8 */
    int32_t   num_strips;     /* in : > 0 */
    uint8_t  *out;            /* in : caller buffer, out_cap >= MIC_HIP_PICS_BOUND(...) is always sufficient */
    size_t    out_cap;        /* in  */
    size_t    out_len;        /* out */
    int32_t   status;         /* out */
    int32_t   failed_strip;   /* out: the first strip whose codec failed (parallelstrips.go:97), -1: none / not a strip's error */
} mic_hip_pics_enc_job;
typedef struct mic_hip_pics_dec_job {
    const uint8_t *compressed; /* in : a PICS file (host memory) */
    size_t    compressed_len;  /* in  */
    uint16_t *pixels_out;      /* in : width*height u16 (host memory) */
    int32_t   width, height;   /* in : must equal the header's */
    int32_t   status;          /* out */
    int32_t   failed_strip;    /* out: the first strip that failed to decode (parallelstrips.go:316), -1: none */
} mic_hip_pics_dec_job;
int mic_hip_pics_compress_batch(mic_hip_pics_enc_job *jobs, int njobs);
int mic_hip_pics_decompress_batch(mic_hip_pics_dec_job *jobs, int njobs);

/* ---- verified encode and CRC-32 digests ---------------------------------------------------------------- */
/* The formats carry no checksum ("No checksums -- caller must verify integrity", fsedecompressu16.go:21-23).  The calls below
 * prove on the device that a stream decodes to the pixels it was made from, and give every unit / image a digest that travels
 * BESIDE the file (an index, a DICOM attribute): the IEEE CRC-32 -- zlib's crc32, Go's hash/crc32.ChecksumIEEE: reflected
 * polynomial 0xEDB88320, init and final xor 0xFFFFFFFF -- of the pixels as little-endian u16 bytes in row-major order. */
typedef struct mic_hip_verify_result {
    int32_t  status;          /* MIC_OK: checked and equal; MIC_ERR_MISMATCH; anything else is the codec's own status: not checked */
    uint32_t crc32;           /* CRC-32 of the REFERENCE pixels (the encoder's input); valid whenever the unit's arguments were */
    uint64_t mismatches;      /* differing samples (0 unless status is MIC_ERR_MISMATCH) */
    int64_t  first_mismatch;  /* smallest differing pixel index within the unit / image, -1: none */
} mic_hip_verify_result;
/* crc(A || B) from crc(A), crc(B) and B's length in bytes (zlib's crc32_combine).  Needs no device. */
uint32_t mic_hip_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);
/* mic_hip_compress_batch / mic_hip_pics_compress_batch with the check: every sub-batch is decoded again on the device from the
 * bytes that were just packed and compared with the pixels it came from, in front of the download.  Files, out_len, failed_strip,
 * sub-batches and devices are those of the unverified calls, byte for byte.  res[j] describes job j as a whole (a PICS image: its
 * strips' CRCs joined in order, mismatches summed, first_mismatch the image's pixel index).  A job that fails the check gets
 * status MIC_ERR_MISMATCH in the job and in res[j] -- failed_strip names its first strip that differed --; its bytes are still
 * delivered and out_len is set, so the caller can keep the evidence.  A job the codec refused keeps that status in both. */
int mic_hip_compress_batch_verified(mic_hip_enc_job *jobs, int njobs, mic_hip_verify_result *res);
int mic_hip_pics_compress_batch_verified(mic_hip_pics_enc_job *jobs, int njobs, mic_hip_verify_result *res);
/* mic_hip_decompress_batch / mic_hip_pics_decompress_batch with the digest of what was decoded: crc[j] = the CRC-32 of job j's
 * pixels, taken on the device in front of the download (0 for a job that did not decode).  expect (may be NULL): a decoded job
 * whose CRC is not expect[j] gets status MIC_ERR_MISMATCH; its pixels are delivered all the same. */
int mic_hip_decompress_batch_crc(mic_hip_dec_job *jobs, int njobs, const uint32_t *expect, uint32_t *crc);
int mic_hip_pics_decompress_batch_crc(mic_hip_pics_dec_job *jobs, int njobs, const uint32_t *expect, uint32_t *crc);

/* Replaces CompressSingleFrameGrad / DecompressSingleFrameGrad (multiframecompress.go:111-142): the unit codec with the
 * gradient-adaptive predictor (deltagradrlecompressu16.go) and the two-state -> one-state FSE chain. */
int mic_hip_compress_frame_grad(const uint16_t *pixels, int width, int height, uint16_t max_value,
                                uint8_t *out, size_t out_cap, size_t *out_len);
int mic_hip_decompress_frame_grad(const uint8_t *compressed, size_t compressed_len,
                                  uint16_t *pixels_out, int width, int height);

/* ---- gap removal: the unit codec with a compact alphabet ------------------------------------------- */
/* Replaces CompressSingleFrameGapRemoval / DecompressSingleFrameGapRemoval (gapremovalcompressu16.go:52-176, :178-282): the
 * Delta+RLE tokens of CompressSingleFrame; when few of the values below the largest one occur (:104-111), the tokens are coded as
 * indices into the sorted list of the values used, and the list goes in front of the FSE stream as a raw list (mode 0x01) or a
 * delta list (0x03); otherwise the file is 0x00 || CompressSingleFrame's bytes.  The decoder also reads the bitmap form (0x02) the
 * reference's encoder never chooses.  nstates = 2 is the reference's encoder byte for byte (two-state FSE, then one-state,
 * :328-339); 4 and 8 apply the chains of CompressSingleFrame4State / 8State (multiframecompress.go:38-95) to the compact tokens --
 * the reference's decoder reads those too (FSEDecompressU16Auto); anything else is MIC_ERR_ARGS.
 * out_cap >= MIC_HIP_GAP_FRAME_BOUND(width*height) is always sufficient: a chosen map is never larger than the bitmap, at most
 * 3 + 8192 bytes.  A malformed map, an empty input and a decoded compact symbol >= numSymbols (:270-273: only a symbol the payload
 * emits counts, not one its NCount merely weights) are MIC_ERR_CORRUPT.  A gap-removal unit of the session API takes a map slab of
 * 24 KiB beside the unit codec's (136 KiB in a session whose slabs are the worst-case ones). */
#define MIC_HIP_GAP_FRAME_BOUND(npx) (MIC_HIP_FRAME_BOUND(npx) + 8195)
int mic_hip_compress_frame_gap(const uint16_t *pixels, int width, int height, uint16_t max_value, int nstates,
                               uint8_t *out, size_t out_cap, size_t *out_len);
int mic_hip_decompress_frame_gap(const uint8_t *compressed, size_t compressed_len, uint16_t *pixels_out, int width, int height);
/* Many frames in one call, through the same pipeline as mic_hip_compress_batch / _decompress_batch (sub-batches, pinned staging,
 * mic_hip_set_devices shards); per-job status and nstates_used as there.  Every job's bytes equal the single-frame call's. */
int mic_hip_compress_batch_gap(mic_hip_enc_job *jobs, int njobs);
int mic_hip_decompress_batch_gap(mic_hip_dec_job *jobs, int njobs);

/* ---- PICA container: content-adaptive strips, per-strip predictor choice ------------------------ */
/* out_cap >= MIC_HIP_PICA_BOUND(width, height, num_strips) is always sufficient: 16 header bytes, 16 per entry, and the kept
 * candidate of every strip within its MIC_HIP_FRAME_BOUND (the strips' pixels add up to the image's). */
#define MIC_HIP_PICA_BOUND(width, height, num_strips) \
    (16 + 16 * (size_t)(num_strips) + 4 * (size_t)(width) * (size_t)(height) + 135168 * (size_t)(num_strips))
/* Replaces CompressParallelStripsAdaptive (parallelstripsadaptive.go:54): strip boundaries by equal-cost partition of the rows'
 * summed |vertical delta| (adaptiveStripBoundaries, :222-289, float64 like the reference), every strip coded with both the avg
 * and the gradient-adaptive predictor (CompressSingleFrame / CompressSingleFrameGrad, two-state FSE) and the smaller kept, ties to
 * the gradient one (:97-105).  num_strips must be given (the reference's default is GOMAXPROCS).  Either predictor is kept at any
 * width: mic_hip_pica_decompress reads gradient strips wider than 32768 columns too (see MIC_HIP_PRED_GRAD). */
int mic_hip_pica_compress(const uint16_t *pixels, int width, int height, uint16_t max_value, int num_strips,
                          uint8_t *out, size_t out_cap, size_t *out_len);
/* The same with the index of the strip the error belongs to (the reference wraps it: "pica: strip %d: %w",
 * parallelstripsadaptive.go:110): the first strip, in strip order, whose kept candidate failed (:95-114) -- a strip fails only when
 * both encodes did, and its error is then the avg one's -- or that has no rows (the partition clamps late boundaries, :282-284:
 * MIC_ERR_ARGS); -1 when the call succeeded or the error is not a strip's. */
int mic_hip_pica_compress_ex(const uint16_t *pixels, int width, int height, uint16_t max_value, int num_strips,
                             uint8_t *out, size_t out_cap, size_t *out_len, int *failed_strip);
int mic_hip_pica_info(const uint8_t *compressed, size_t compressed_len, int *width, int *height, int *num_strips);
/* Replaces DecompressParallelStripsAdaptive (parallelstripsadaptive.go:141).  Rows no strip covers come back zero (:175). */
int mic_hip_pica_decompress(const uint8_t *compressed, size_t compressed_len, uint16_t *pixels_out, int width, int height);
/* ... and with the index of the strip that failed to decode ("pica: strip %d: %w", :207; -1: none). */
int mic_hip_pica_decompress_ex(const uint8_t *compressed, size_t compressed_len, uint16_t *pixels_out, int width, int height,
                               int *failed_strip);
/* Many images, one call, through the pipeline of mic_hip_pics_compress_batch (sub-batches, pinned staging, mic_hip_set_devices
 * shards by pixels): the reference reaches this by calling CompressParallelStripsAdaptive from many goroutines, each fanning out
 * two encodes per strip (:86-108).  Row costs and boundaries of all images of a sub-batch are found on the device, both candidates
 * of every strip run in one unit batch, the winner is picked there and only it is packed and downloaded.  Every job's file equals
 * mic_hip_pica_compress's, byte for byte; a job with bad arguments or a failing strip fails alone. */
typedef struct mic_hip_pica_enc_job {
    const uint16_t *pixels;   /* in : width*height u16 (host memory) */
    int32_t   width, height;  /* in  */
    uint16_t  max_value;      /* in  (two-state FSE only: :90-92) */
    int32_t   num_strips;     /* in : > 0 */
    uint8_t  *out;            /* in : caller buffer, out_cap >= MIC_HIP_PICA_BOUND(...) is always sufficient */
    size_t    out_cap;        /* in  */
    size_t    out_len;        /* out */
    int32_t   status;         /* out */
    int32_t   failed_strip;   /* out: as mic_hip_pica_compress_ex */
} mic_hip_pica_enc_job;
typedef struct mic_hip_pica_dec_job {
    const uint8_t *compressed; /* in : a PICA file (host memory) */
    size_t    compressed_len;  /* in  */
    uint16_t *pixels_out;      /* in : width*height u16 (host memory) */
    int32_t   width, height;   /* in : must equal the header's */
    int32_t   status;          /* out */
    int32_t   failed_strip;    /* out: the first strip that failed to decode, -1: none */
} mic_hip_pica_dec_job;
int mic_hip_pica_compress_batch(mic_hip_pica_enc_job *jobs, int njobs);
int mic_hip_pica_decompress_batch(mic_hip_pica_dec_job *jobs, int njobs);
/* adaptiveStripBoundaries alone (:222-289): starts[0 .. *n_out) of one image, n_out = min(num_strips, height) <= cap.
 * on_host = 0: the device's partition kernel, as the batch uses it; 1: the reference's float64 loop on the host, fed with the
 * device's row costs -- the two agree for every input (tests/test_gpu_pica_batch.py). */
int mic_hip_pica_boundaries(const uint16_t *pixels, int width, int height, int num_strips, int on_host,
                            int32_t *starts, int cap, int *n_out);

/* ---- MIC2 container, independent frames --------------------------------------------------- */
/* Replaces CompressMultiFrame(..., temporal=false) (multiframecompress.go:179) +
 * WriteMIC2 (multiframe.go:49).  frames = nframes*width*height u16, frame-major.  out_cap >= MIC_HIP_MIC2_BOUND(...) is always
 * sufficient (also for the temporal form below). */
int mic_hip_mic2_compress(const uint16_t *frames, int width, int height, int nframes,
                          uint16_t max_value,
                          uint8_t *out, size_t out_cap, size_t *out_len);
/* CompressMultiFrame(frames, w, h, maxValue, temporal=true) + WriteMIC2 (multiframecompress.go:179-224,
 * temporaldelta.go:11-23): frame 0 spatial, frame i > 0 = RLE + FSE(2-state, 1-state fallback) of
 * ZigZag(frame i - frame i-1).  Flags byte 0x03.  mic_hip_mic2_decompress reads both pipelines. */
int mic_hip_mic2_compress_temporal(const uint16_t *frames, int width, int height, int nframes,
                                   uint16_t max_value, uint8_t *out, size_t out_cap, size_t *out_len);
int mic_hip_mic2_info(const uint8_t *compressed, size_t compressed_len,
                      int *width, int *height, int *nframes, int *temporal);
/* Replaces DecompressMultiFrame (multiframecompress.go:227) for independent-mode files. */
int mic_hip_mic2_decompress(const uint8_t *compressed, size_t compressed_len,
                            uint16_t *frames_out, size_t frames_cap_px);
/* DecompressFrame(data, frameIdx) (multiframecompress.go:266-315) with ExtractFrame (multiframe.go:131-142):
 * one frame of a MIC2 file; temporal files decode frames 0..frame_idx. */
int mic_hip_mic2_decompress_frame(const uint8_t *compressed, size_t compressed_len, int frame_idx,
                                  uint16_t *pixels_out, size_t pixels_cap);

/* Many volumes per call (no reference counterpart: CompressMultiFrame / DecompressMultiFrame, multiframecompress.go:179-261, and
 * WriteMIC2 / ReadMIC2, multiframe.go:49-142, of each job).  A dataset of small volumes -- cine loops, NM and tomosynthesis stacks --
 * pays one entropy chain per volume through the single calls, and a chain costs about the same for 30 units as for 2304.  Here one
 * call may mix volumes of any width, height, frame count and bit depth, independent (temporal = 0) and temporal (1:
 * TemporalDeltaEncode / TemporalDeltaDecode, temporaldelta.go:11-37) ones; the units of all of them -- volume order, then frame
 * order -- go through the unit codec in shared sub-batches cut under the workspace ceiling by the units' sizes alone (the rule of
 * mic_hip_mic2_multi_read_crops; mic_hip_mic2_batch_plan states it): a cut may fall between volumes or inside one, frames, frame 0 of
 * temporal volumes and residual units share a sub-batch, and when everything fits one sub-batch the call runs ONE chain
 * (stats->slabs == 1).  Every file written equals the file mic_hip_mic2_compress / mic_hip_mic2_compress_temporal writes for that
 * volume, byte for byte; every decode equals mic_hip_mic2_decompress.
 * Returns MIC_OK when the batch ran; njobs == 0 is MIC_OK with zeroed stats; MIC_ERR_ARGS for njobs < 0 or jobs NULL.
 * A volume fails alone, with the single call's code in status: bad arguments (MIC_ERR_ARGS), more than 2^28 pixels a frame
 * (MIC_ERR_UNSUPPORTED), a buffer too small (MIC_ERR_CAPACITY), a header mic_hip_mic2_info refuses (its code; a dimension of 0:
 * MIC_ERR_CORRUPT), a table entry of length 0 or outside the file (MIC_ERR_CORRUPT), a frame the unit codec refuses (its code), a
 * payload over the u32 offsets (MIC_ERR_UNSUPPORTED, multiframe.go:75-80).  failed_frame is the first failing frame in frame order,
 * -1 when the error is not a frame's.  A failed encode job has out_len 0, a failed decode job's pixels are unspecified, every other
 * volume is exact; a temporal volume's failed frame stops only that volume.
 * The sub-batches are the parts of the host pipeline: part k + 1 comes up while part k is coded and part k - 1 goes down; pinned
 * buffers (mic_hip_host_alloc) are sent in place.  A part that starts inside a temporal volume uploads the ORIGINAL frame in front of
 * it on encode, and on decode takes the running sum from where the part before left that frame on the device.
 * mic_hip_set_devices shards the volumes by pixels, a shard boundary between volumes only; each shard cuts its own units.
 * stats (may be NULL): units = the frames of the volumes whose arguments (decode: header and table) were accepted, slabs = the
 * chains the call ran, volumes_done = the volumes whose status is MIC_OK. */
typedef struct mic_hip_mic2_enc_job {
    const uint16_t *frames;            /* in : nframes*width*height u16, frame-major (host) */
    int32_t  width, height, nframes;   /* in  */
    uint16_t max_value;                /* in  */
    uint16_t temporal;                 /* in : 0 independent, 1 temporal */
    uint8_t *out; size_t out_cap;      /* in : MIC_HIP_MIC2_BOUND(...) always suffices */
    size_t   out_len;                  /* out */
    int32_t  status, failed_frame;     /* out: first failing frame, -1 when not a frame's error */
} mic_hip_mic2_enc_job;
typedef struct mic_hip_mic2_dec_job {
    const uint8_t *compressed; size_t compressed_len;   /* in (host) */
    uint16_t *frames_out; size_t frames_cap_px;          /* in (host) */
    int32_t  width, height, nframes, temporal;           /* out: the header's (0 when the header was refused) */
    int32_t  status, failed_frame;                       /* out */
} mic_hip_mic2_dec_job;
typedef struct { uint64_t units, slabs, volumes_done; } mic_hip_mic2_batch_stats;
int mic_hip_mic2_compress_batch(mic_hip_mic2_enc_job *jobs, int njobs, mic_hip_mic2_batch_stats *stats);
int mic_hip_mic2_decompress_batch(mic_hip_mic2_dec_job *jobs, int njobs, mic_hip_mic2_batch_stats *stats);
/* The cut rule of those calls as a host function: whn = (width, height, nframes) of nvol volumes; their units, volume by volume and
 * frame by frame, are cut into sub-batches -- a sub-batch takes units while their number stays within
 * budget_bytes / (tier-2 slabs of its largest frame + that frame's pixels) and within 65535, at least one.  budget_bytes == 0: the
 * default ceiling (MIC_HIP_WS_BUDGET_MB, else from the device's memory).  cuts[0 .. *ncuts) receives 0, ..., *nunits: sub-batch b is
 * units cuts[b] .. cuts[b + 1] - 1, so a call over these volumes runs *ncuts - 1 chains (no volumes: cuts = { 0 }).  cap short:
 * MIC_ERR_CAPACITY with the counts set and cuts untouched; a dimension <= 0: MIC_ERR_ARGS.  Needs no device. */
int mic_hip_mic2_batch_plan(const int32_t *whn, int nvol, size_t budget_bytes,
                            uint32_t *cuts, size_t cap, uint64_t *ncuts, uint64_t *nunits);
/* (the device-resident forms, mic_hip_session_mic2_encode / _decode, stand with the session calls) */

/* Many 3-D crops per call, into a tensor that already lives on the device (no reference counterpart; beside
 * mic_hip_mic2_decompress / _decompress_frame, which serve whole frames through the host, and the MIC3 patch calls, whose semantics
 * carry over).  Crop i is the box [x, x + cw) x [y, y + ch) x [z, z + cd) with (x, y, z) = xyz[3i .. 3i + 2], z the frame index;
 * origins may be negative and a box may overhang the volume in any axis or lie wholly outside it: samples outside the volume are
 * 0.  d_out receives n x cd x ch x cw little-endian u16 -- crop-major, then frame, row, column --, n * cd * ch * cw * 2 bytes, every
 * one of them written.  d_out is memory the device can write: a device allocation on the call's device that is long enough for
 * the tensor, or pinned host memory (mic_hip_host_alloc); anything else is MIC_ERR_ARGS, found with hipPointerGetAttributes before
 * anything is launched.
 * Independent files: only the frames some crop overlaps are entropy-decoded, each once, and a kernel writes every (crop, frame)
 * overlap -- a "piece" -- from the decoded frames into d_out.  Temporal files: frame_i = frame_0 + sum UnZigZag(res_j) mod 2^16 is
 * summed under the crops' footprints only, by a kernel that walks the residual symbols and stores the crop slices; frames 1.. never
 * exist as images, and residual streams behind the last frame a crop overlaps are not decoded.  Both run in sub-batches of frames
 * under the workspace ceiling.
 * status[i] (host, may be NULL): MIC_OK, or the unit codec's code of the first failing frame, in frame order, among the frames
 * crop i depends on -- independent: the frames it overlaps with non-empty area; temporal: frames 0 .. the last one it overlaps (a
 * damaged residual poisons everything behind it).  Such a crop's samples are unspecified, every other crop is exact.
 * Returns MIC_OK when the call ran, even if crops failed; n == 0 is MIC_OK; MIC_ERR_ARGS for cw, ch, cd <= 0 or n < 0;
 * MIC_ERR_CAPACITY for out_cap below the tensor's size; the header's and table's errors are mic_hip_mic2_info's; a table entry of a
 * needed frame that has length 0 or points outside the file fails the whole call with MIC_ERR_CORRUPT, as mic_hip_mic2_decompress
 * does.  One device: the calling thread's default session (the file and reader forms) or the given session; no fan-out over
 * mic_hip_set_devices.
 * stats (may be NULL): frames entropy-decoded and pieces (the plan's counts), slabs = decode chains the call ran. */
typedef struct { uint64_t frames_decoded, pieces, slabs; } mic_hip_crop_stats;
/* The host planner of those calls: frames[cap] receives the frames whose streams must be entropy-decoded, ascending, each once --
 * independent (temporal = 0): the union of the frames the crops overlap; temporal: 0 .. the last overlapped frame; none when no
 * crop has a non-empty overlap.  *nframes_out their number, *npieces the number of (crop, frame) pairs with non-empty overlap area,
 * in both modes (both may be NULL).  More than cap frames: MIC_ERR_CAPACITY with the counts set and frames untouched.  Needs no
 * device. */
int mic_hip_mic2_crop_plan(int width, int height, int nframes, int temporal,
                           const int32_t *xyz, int n, int cw, int ch, int cd,
                           uint32_t *frames, size_t cap, uint64_t *nframes_out, uint64_t *npieces);
int mic_hip_mic2_read_crops(const uint8_t *compressed, size_t compressed_len,
                            const int32_t *xyz, int n, int cw, int ch, int cd,
                            void *d_out, size_t out_cap, int32_t *status, mic_hip_crop_stats *stats);
/* (the reader form, mic_hip_mic2_reader_*, stands with the streaming calls below, the session form,
 * mic_hip_session_mic2_read_crops, with the session calls: they need those sections' types) */

/* Crops of many volumes per call: a training batch takes each box from another volume of the dataset, and a call per volume pays a
 * whole decode chain per box.  The semantics of the calls above carry over except as stated.  Crop i is (x, y, z, volume) =
 * xyzv[4i .. 4i + 3], the box [x, x + cw) x [y, y + ch) x [z, z + cd) of files[volume].  One call may mix volumes of any width, height,
 * frame count and bit depth, independent and temporal files, and list a volume twice (it is then two volumes).
 * The frames the crops need, of all volumes, go through the unit codec in plan order -- ascending by volume, then frame -- in
 * sub-batches cut under the workspace ceiling by the frames' sizes alone: a cut may fall between volumes or inside one, frames of
 * independent volumes, frame 0 of temporal ones and residual units share a sub-batch, and when everything fits one sub-batch the call
 * runs ONE decode chain (stats->slabs == 1).
 * Before a file is looked at and before anything is launched, d_out untouched, in this order: MIC_ERR_ARGS for cw, ch, cd <= 0, n < 0,
 * nfiles < 0 or a NULL array that is needed; MIC_ERR_CAPACITY for out_cap below the tensor's size; MIC_ERR_ARGS for a volume index
 * outside [0, nfiles); MIC_ERR_ARGS for d_out NULL or not memory the call's device can write.  n == 0 is MIC_OK with zeroed stats.
 * A volume fails alone: status[i] of every crop of it gets the volume's code, those crops are all 0 and no other volume is affected
 * -- a NULL file or reader (MIC_ERR_ARGS), a header mic_hip_mic2_info refuses (its code; width or height 0: MIC_ERR_CORRUPT), more than
 * 2^28 pixels a frame or a file longer than 0xFFFFFFF0 (MIC_ERR_UNSUPPORTED), in the session form a head shorter than 20 + 8 * nframes
 * or a NULL d_files entry of a volume whose frames are needed (MIC_ERR_ARGS), a table entry of a needed frame with length 0 or a range
 * outside the file (MIC_ERR_CORRUPT -- on purpose not the single-file call's way, which fails as a whole: a batch over a dataset must
 * not die for one bad file).  Volumes no crop names are not parsed and not read; they may be NULL or garbage.
 * status[i] (may be NULL) is otherwise MIC_OK or the unit codec's code of the first failing frame, in frame order, among the frames
 * crop i depends on (independent: the frames it overlaps; temporal: 0 .. the last it overlaps); failed_frame[i] (may be NULL) that
 * frame, else -1, also for a volume-level failure.  A failed crop's samples are unspecified, every other crop is exact; a temporal
 * volume's failed frame stops only that volume.  Returns MIC_OK when the call ran.
 * stats (may be NULL): frames_decoded and pieces are the planner's counts, slabs the decode chains the call ran, volumes_read the
 * named volumes whose header and needed table entries were accepted. */
typedef struct { uint64_t frames_decoded, pieces, slabs, volumes_read; } mic_hip_multi_crop_stats;
/* The host planner: volume_of[cap] / frame_of[cap] receive the (volume, frame) units whose streams must be entropy-decoded, ascending
 * by volume, then frame, each once -- independent volume: the overlapped frames; temporal: 0 .. the last overlapped frame.
 * *nframes_out their number, *npieces the (crop, frame) overlaps with non-empty area (both may be NULL); file_status[nfiles] (may be
 * NULL) each volume's code as above, MIC_OK for a volume no crop names.  More than cap units: MIC_ERR_CAPACITY with the counts and
 * file_status set and the arrays untouched; more than 2^32 - 1 pieces: MIC_ERR_UNSUPPORTED.  Reads only the 20-byte headers and the
 * frame tables.  Needs no device. */
int mic_hip_mic2_multi_crop_plan(const uint8_t *const *files, const size_t *lens, int nfiles,
                                 const int32_t *xyzv, int n, int cw, int ch, int cd,
                                 uint32_t *volume_of, uint32_t *frame_of, size_t cap,
                                 uint64_t *nframes_out, uint64_t *npieces, int32_t *file_status);
int mic_hip_mic2_multi_read_crops(const uint8_t *const *files, const size_t *lens, int nfiles,
                                  const int32_t *xyzv, int n, int cw, int ch, int cd, void *d_out, size_t out_cap,
                                  int32_t *status, int32_t *failed_frame, mic_hip_multi_crop_stats *stats);
/* (mic_hip_mic2_readers_read_crops stands with the streaming calls, mic_hip_session_mic2_multi_read_crops with the session calls) */

/* ---- strip files: many crops per call --------------------------------------------------------- */
/* Many 2-D crops of many PICS / PICA files per call, into a tensor that already lives on the device (no reference counterpart;
 * beside mic_hip_pics_decompress_batch / mic_hip_pica_decompress_batch, which serve whole images through the host, and the MIC3 patch
 * and MIC2 crop calls, whose semantics carry over).  files[f] (lens[f] bytes, host memory) is a PICS or a PICA file, told apart by its
 * magic; one call may mix the two kinds, any sizes, strip counts and state flavours.  Crop i is the rectangle [x, x + cw) x [y, y + ch)
 * of file xyf[3i + 2], (x, y) = xyf[3i .. 3i + 1]; origins may be negative and a crop may overhang its image or lie wholly outside
 * it: samples outside the image are 0, and so are rows no strip of the header covers, as the whole-image decoders return them.
 * d_out receives n x ch x cw little-endian u16 -- crop-major, then row, column --, n * ch * cw * 2 bytes, every one of them written.
 * d_out is memory the device can write: a device allocation on the call's device that is long enough for the tensor, or pinned host
 * memory (mic_hip_host_alloc); anything else is MIC_ERR_ARGS, found with hipPointerGetAttributes before anything is launched.
 * A strip is a unit of its own, so only the strips some crop overlaps with non-empty area are uploaded and entropy-decoded, each
 * once, in sub-batches under the workspace ceiling, each into a slab of decoded strips; behind each sub-batch a kernel writes every
 * (crop, strip) overlap -- a "piece" -- from the slab into d_out.  A strip is decoded whole, whatever part of it a crop needs.
 * A file fails alone: one whose header or table mic_hip_pics_info / mic_hip_pica_info refuse, or with an entry the whole-image
 * decoders refuse -- a byte range outside the file, an empty or inverted row range, length 0 (all MIC_ERR_CORRUPT), a strip of more
 * than 2^28 pixels (MIC_ERR_UNSUPPORTED) --, or whose pointer is NULL (MIC_ERR_ARGS), gives that code to status[i] of every crop of
 * it, and those crops are all zero; no other file is affected.  Files no crop names are not looked at.
 * status[i] (host, may be NULL) is otherwise MIC_OK, or the unit codec's code of the first failing strip, in strip order, among
 * the strips crop i overlaps with non-empty area; failed_strip[i] (host, may be NULL) that strip's index, else -1.  Such a crop's
 * samples are unspecified, every other crop is exact.
 * Returns MIC_OK when the call ran, even if crops failed; n == 0 is MIC_OK; before anything is launched MIC_ERR_ARGS for cw, ch <= 0,
 * n < 0, nfiles < 0, a NULL array or a file index outside [0, nfiles), and MIC_ERR_CAPACITY for out_cap below the tensor's size.
 * One device: the calling thread's default session, or the given session (mic_hip_session_strips_read_crops, with the session
 * calls below); no fan-out over mic_hip_set_devices.  There is no callback-reader form: a strip file's table is a few hundred
 * bytes, and its reader would be the file form.
 * stats (may be NULL): strips entropy-decoded and pieces (the plan's counts), strips_total = the strips of the files some crop
 * names, refused files left out (what whole-image decodes of them would run), slabs = decode chains the call ran. */
typedef struct { uint64_t strips_decoded, strips_total, pieces, slabs; } mic_hip_strip_crop_stats;
/* The host planner of those calls: file_of[cap] / strip_of[cap] receive the (file, strip) units whose streams must be
 * entropy-decoded -- the strips some crop overlaps with non-empty area --, ascending by file, then strip, each once.  *nstrips_out
 * their number, *npieces the number of (crop, strip) overlaps with non-empty area (both may be NULL).  file_status[nfiles] (may be
 * NULL): the code of each file as above; MIC_OK for a file no crop names.  More than cap units: MIC_ERR_CAPACITY with the counts
 * and file_status set and the arrays untouched.  Only the files' headers and tables are read.  Needs no device. */
int mic_hip_strips_crop_plan(const uint8_t *const *files, const size_t *lens, int nfiles,
                             const int32_t *xyf, int n, int cw, int ch,
                             uint32_t *file_of, uint32_t *strip_of, size_t cap,
                             uint64_t *nstrips_out, uint64_t *npieces, int32_t *file_status);
int mic_hip_strips_read_crops(const uint8_t *const *files, const size_t *lens, int nfiles,
                              const int32_t *xyf, int n, int cw, int ch,
                              void *d_out, size_t out_cap,
                              int32_t *status, int32_t *failed_strip, mic_hip_strip_crop_stats *stats);

/* ---- single-frame RGB files: many crops of many files per call, written to a device tensor ------ */
/* The same for CompressRGB blobs and MICR files (below; no reference counterpart): a sampler that feeds a model cw x ch crops of
 * ultrasound frames or visible-light images otherwise decodes whole images (mic_hip_rgb_decompress_batch), crops on the host and
 * uploads crop by crop.  files[f] is a blob with its width and height, or a MICR file (width = height = 0: the header's; else they
 * must equal it); one call may mix the two kinds and any sizes.  Crop i is the rectangle [x, x + cw) x [y, y + ch) of file
 * xyf[3i + 2], (x, y) = xyf[3i .. 3i + 1]; origins may be negative and a crop may overhang its image or lie wholly outside it:
 * samples outside the image are 0.  d_out receives n x ch x cw x 3 interleaved u8 -- crop-major, then row, column, channel --,
 * n * ch * cw * 3 bytes at any address, every one of them written.  d_out is memory the device can write: a device allocation on the
 * call's device that is long enough for the tensor, or pinned host memory (mic_hip_host_alloc); anything else is MIC_ERR_ARGS, found
 * with hipPointerGetAttributes before anything is launched.
 * An image is one unit of the plan, so only the files some crop overlaps with non-empty area are looked at, uploaded and decoded,
 * each once and whole, in sub-batches under the workspace ceiling; a file no crop names that way is not looked at beyond a MICR
 * file's 12-byte header.  A sub-batch's slab holds the CODED planes alone (plane mode 2: an entropy-coded stream), and the cut counts
 * only their samples: a grey ultrasound frame codes Y and has constant Co and Cg, so three times as many of them share one decode
 * chain as full-colour images do.  Behind each sub-batch one kernel writes every (crop, image) overlap -- a "piece", at most one per
 * crop -- into d_out, taking each plane from where it is: the decoded plane in the slab, the constant of a mode 0 / 1 plane from
 * the piece's record, the raw samples of a mode 3 plane in place from the uploaded blob.  No constant or raw plane is materialised.
 * A file fails alone, with the code and failed_plane mic_hip_rgb_decompress_batch gives the same file: a NULL pointer, a width or
 * height < 0, 0 for a blob, or that disagrees with a MICR header, a container that is neither 0 nor 1 (MIC_ERR_ARGS), more than 2^26
 * pixels (MIC_ERR_UNSUPPORTED), a MICR header mic_hip_micr_info refuses, a blob whose lengths or plane modes decompressRGBTileBlob
 * refuses (MIC_ERR_CORRUPT).  Every crop of such a file gets that code, and its pixels are zero; no other file is affected.
 * status[i] (host, may be NULL) is otherwise MIC_OK, or the unit codec's code of the first failing plane of crop i's file, in plane
 * order; failed_plane[i] (host, may be NULL) that plane (0 Y, 1 Co, 2 Cg), else -1.  Such a crop's samples are unspecified, every
 * other crop is exact.
 * Returns MIC_OK when the call ran, even if crops failed; n == 0 is MIC_OK; before anything is launched MIC_ERR_ARGS for cw, ch <= 0,
 * n < 0, nfiles < 0, a NULL array or a file index outside [0, nfiles), and MIC_ERR_CAPACITY for out_cap below the tensor's size.
 * One device: the calling thread's default session, or the given session (mic_hip_session_rgb_read_crops, with the session calls
 * below); no fan-out over mic_hip_set_devices.  There is no callback-reader form: a blob is one unit, its reader would be the file form.
 * stats (may be NULL): planes_decoded = the mode 2 planes that were entropy-decoded, planes_total = 3 x the accepted files some crop
 * names (what whole-image decodes of them would lay out), pieces = the crops with non-empty overlap, slabs = decode chains the call ran. */
typedef struct mic_hip_rgb_file {
    const uint8_t *data; size_t len;   /* a CompressRGB blob or a MICR file (host memory) */
    int32_t width, height;             /* blob: the image's.  MICR: 0 = take the header's, else must equal it */
    int32_t container;                 /* 0: CompressRGB blob, 1: MICR file */
} mic_hip_rgb_file;
typedef struct { uint64_t planes_decoded, planes_total, pieces, slabs; } mic_hip_rgb_crop_stats;
/* The host planner of those calls: file_of[cap] receives the files whose planes must be decoded -- the accepted files some crop
 * overlaps with non-empty area --, ascending and each once.  *nfiles_out their number, *nplanes_coded their mode 2 planes,
 * *npieces the crops with non-empty overlap of them (each may be NULL).  file_status[nfiles] (may be NULL): the code of each file as
 * above; MIC_OK for a file no crop names.  More than cap files: MIC_ERR_CAPACITY with the counts and file_status set and the array
 * untouched.  Of a named file only the three lengths and the first bytes of each plane are read.  Needs no device. */
int mic_hip_rgb_crop_plan(const mic_hip_rgb_file *files, int nfiles, const int32_t *xyf, int n, int cw, int ch,
                          uint32_t *file_of, size_t cap, uint64_t *nfiles_out, uint64_t *nplanes_coded, uint64_t *npieces,
                          int32_t *file_status);
int mic_hip_rgb_read_crops(const mic_hip_rgb_file *files, int nfiles, const int32_t *xyf, int n, int cw, int ch,
                           void *d_out, size_t out_cap, int32_t *status, int32_t *failed_plane, mic_hip_rgb_crop_stats *stats);

/* ---- WaveletV2 -------------------------------------------------------------------------------- */
/* Replaces WaveletV2RLEFSECompressU16 and WaveletV2SIMDRLEFSECompressU16 (waveletfsecompressu16.go:303,
 * :374; identical streams): up to 8 levels of 5/3 integer lifting in Mallat layout, subband scan, zigzag
 * with 3-word escape, RLE with length prefix, 4-state FSE (no fallback), 11-byte header.
 * NOTE the argument order of the reference: (pixels, rows, cols, maxValue, levels). */
int mic_hip_wavelet_v2_compress(const uint16_t *pixels, int rows, int cols, uint16_t max_value, int levels,
                                uint8_t *out, size_t out_cap, size_t *out_len);
int mic_hip_wavelet_v2_info(const uint8_t *compressed, size_t compressed_len,
                            int *rows, int *cols, int *max_value, int *levels);
/* Replaces WaveletV2RLEFSEDecompressU16 / WaveletV2SIMDRLEFSEDecompressU16 (:380, :493). */
int mic_hip_wavelet_v2_decompress(const uint8_t *compressed, size_t compressed_len,
                                  uint16_t *pixels_out, size_t out_cap_px);

/* Many frames of one shape side by side (the reference codes one image per call; a WaveletV2 file is ONE serial 4-state FSE
 * stream, so a single decode is one wave walking one chain -- the device pays off when frames are coded together).
 * compress_batch: frames = nframes x rows*cols u16, contiguous; frame i's file (byte-identical to the single call's) is written at
 * out + i*out_stride, out_lens[i] / status[i] per frame; a failing frame does not stop the others.
 * decompress_batch: nframes files of ONE shape (rows, cols, levels of files[0]; others: status MIC_ERR_ARGS); pixels_out receives
 * nframes x rows*cols u16. */
int mic_hip_wavelet_v2_compress_batch(const uint16_t *frames, int nframes, int rows, int cols, uint16_t max_value, int levels,
                                      uint8_t *out, size_t out_stride, size_t *out_lens, int32_t *status);
int mic_hip_wavelet_v2_decompress_batch(const uint8_t *const *files, const size_t *lens, int nframes,
                                        uint16_t *pixels_out, size_t out_cap_px, int32_t *status);

/* At reduced resolution (no reference counterpart; the subband scan makes the format resolution-scalable).  For 0 <= level <= levels
 * (the header's level count): nr[0] = rows, nr[l + 1] = (nr[l] + 1) / 2, nc alike; the image at `level` is the nr[level] x nc[level]
 * LL band the forward transform holds after `level` levels, saturated to [0, 65535] (level 0: the decoded image, byte for byte).
 * It needs only the first nr[level] * nc[level] coefficients of the subband scan, so the serial tANS chain stops early: about 1/4^level
 * of the work.  A preview validates only the part of the stream it decodes.
 * level_info (host only): the band's size.  level < 0 or > levels: MIC_ERR_ARGS; a header shorter than 11 bytes: MIC_ERR_CORRUPT.
 * decompress_level_batch: the shape rules of decompress_batch; frame i's band goes to pixels_out + i * nr[level] * nc[level]
 * (capacity checked against that size); symbols_decoded (nullable): the tANS symbols the chain decoded per frame -- a frame whose
 * prefix fell short (escape-heavy 16-bit content) is decoded again whole, and both passes count. */
int mic_hip_wavelet_v2_level_info(const uint8_t *compressed, size_t compressed_len, int level, int *out_rows, int *out_cols);
int mic_hip_wavelet_v2_decompress_level(const uint8_t *compressed, size_t compressed_len, int level,
                                        uint16_t *pixels_out, size_t out_cap_px);
int mic_hip_wavelet_v2_decompress_level_batch(const uint8_t *const *files, const size_t *lens, int nframes, int level,
                                              uint16_t *pixels_out, size_t out_cap_px, int32_t *status, uint64_t *symbols_decoded);

/* Frames of ANY shapes and level counts in one call (no reference counterpart: WaveletV2RLEFSECompressU16 / ...DecompressU16,
 * waveletfsecompressu16.go:303-534, of every job).  A directory mixes shapes and level counts, and a WaveletV2 file is one serial tANS
 * stream: grouped by shape on the host, a group of three frames pays the launch chain's latency as 256 frames do.  Here every launch is
 * driven by a table of the frames -- a 2 x 2 frame beside a 2140 x 1760 one costs one block -- and a frame takes part in the transform
 * levels it has.
 * A job's file equals mic_hip_wavelet_v2_compress's byte for byte (levels_applied: the level count its header carries, :321-330); a
 * decoded job equals mic_hip_wavelet_v2_decompress's, or -- level > 0 -- mic_hip_wavelet_v2_decompress_level's: out_rows x out_cols =
 * nr[level] x nc[level] pixels, row stride out_cols.  The calls return MIC_OK when the batch ran; a job with bad arguments
 * (MIC_ERR_ARGS: a null pointer, a side <= 0, level < 0 or > the header's levels), a shape over 2^27 pixels (MIC_ERR_UNSUPPORTED), a
 * buffer too small (MIC_ERR_CAPACITY), a file shorter than 13 bytes, with a bad header or no four-state stream (MIC_ERR_CORRUPT), or a
 * frame the FSE stage refuses fails alone with its code in `status` and does not move its neighbours' outputs.
 * The jobs are cut into sub-batches (mic_hip_wavelet_v2_batch_plan) that run one launch chain each, their transfers beside the
 * neighbours' kernels; buffers from mic_hip_host_alloc are sent in place; with several devices (mic_hip_set_devices) the jobs are
 * shared out by pixels.  Every unit of a sub-batch is laid out by its largest frame (the tier-2 slabs of this path are not tiered),
 * which the cut rule bounds.
 * stats (nullable): sub_batches = the sub-batches run, chains = the launch chains (one per sub-batch, one more for each sub-batch whose
 * reduced decode sent frames round again whole), frames_done = jobs with MIC_OK, redo_frames = the frames decoded twice. */
typedef struct mic_hip_wv_enc_job {
    const uint16_t *pixels; int32_t rows, cols; uint16_t max_value; int32_t levels;   /* in  */
    uint8_t *out; size_t out_cap;                                                     /* in  */
    size_t out_len; int32_t status; int32_t levels_applied;                           /* out */
} mic_hip_wv_enc_job;
typedef struct mic_hip_wv_dec_job {
    const uint8_t *compressed; size_t compressed_len; int32_t level;                  /* in: 0 = full image */
    uint16_t *pixels_out; size_t out_cap_px;                                          /* in  */
    int32_t rows, cols, levels;       /* out: the header's (0 when refused) */
    int32_t out_rows, out_cols;       /* out: what was written, nr[level] x nc[level] */
    int32_t status; uint64_t symbols_decoded;                                         /* out */
} mic_hip_wv_dec_job;
typedef struct { uint64_t sub_batches, chains, frames_done, redo_frames; } mic_hip_wv_batch_stats;
int mic_hip_wavelet_v2_compress_jobs  (mic_hip_wv_enc_job *jobs, int njobs, mic_hip_wv_batch_stats *stats);
int mic_hip_wavelet_v2_decompress_jobs(mic_hip_wv_dec_job *jobs, int njobs, mic_hip_wv_batch_stats *stats);
/* The cut of the calls above (host only, needs no device): rc = nframes x (rows, cols); a sub-batch takes frames in order while they
 * stay within budget_bytes / (workspace of a unit of the largest frame so far + its planes), 65535 frames and 2^30 pixels; the first
 * frame always joins.  budget_bytes 0: the calls' own ceiling.  cuts[0 .. *ncuts) = 0, ..., nframes; more than `cap`:
 * MIC_ERR_CAPACITY with *ncuts set; a side <= 0: MIC_ERR_ARGS. */
int mic_hip_wavelet_v2_batch_plan(const int32_t *rc, int nframes, size_t budget_bytes,
                                  uint32_t *cuts, size_t cap, uint64_t *ncuts);

/* ---- MIC3 container: tiled RGB whole-slide images ---------------------------------------------- */
/* Replaces CompressWSI (wsicompress.go:27) + WriteMIC3 (wsiformat.go:99) for 8-bit RGB with the
 * YCoCg-R colour transform (forced on for RGB, wsiformat.go:93-95).  tile_w / tile_h = 0 select the
 * 256 x 256 default, levels <= 0 the automatic pyramid depth (wsiformat.go:273-285).  The pyramid
 * (2x2 box, wsipyramid.go:10-32), tile extraction, colour transform, plane statistics and every
 * plane's CompressSingleFrame run on the device; the host writes the container. */
int mic_hip_wsi_compress(const uint8_t *rgb, int width, int height, int tile_w, int tile_h, int levels,
                         uint8_t *out, size_t out_cap, size_t *out_len);
/* CompressWSI(pixels, width, height, channels, bitsPerSample, opts) with the reference's full signature: channels 3 /
 * 8 bits is the call above; channels 1 with 8 or 16 bits per sample (16-bit samples little-endian, bytesToUint16Slice,
 * wsicompress.go:573-587) is the greyscale path -- Downsample2xGrey (wsipyramid.go:34-55), one plane per tile and the tile blob is
 * that plane's blob (compressGreyTileBlob, :366-370), no colour-transform flag.  Other combinations: MIC_ERR_UNSUPPORTED.
 * Several devices (mic_hip_set_devices; not in a nested call) -- the tile worker pool of wsicompress.go:126-145 over GPUs: the slide
 * is cut into one band of tile rows per device (mic_hip_wsi_band_plan).  Every band but the last is a multiple of tile_h << K rows,
 * so it holds whole tiles of levels 0..K and the 2x2 box filter never crosses its edge: each device uploads only its rows and codes
 * levels 0..K of its band as a slide of its own.  The bands' rows of level K + 1 (of level K for an odd tile_h) are staged through
 * pinned host memory to devices[0], which codes levels K + 1 .. L - 1.  All tile lengths are gathered first; out_cap is checked
 * before any byte of `out` is written; each device's tiles are then copied to their final offsets.  The file is byte-identical
 * to the one-device file.  One device, or fewer than two non-empty bands: the one-device path. */
int mic_hip_wsi_compress_ex(const uint8_t *pixels, int width, int height, int channels, int bits_per_sample,
                            int tile_w, int tile_h, int levels, uint8_t *out, size_t out_cap, size_t *out_len);
/* WSIHeader.Channels / BitsPerSample / ColorTransform (wsiformat.go:169-227).  The decompress calls below write
 * channels * (bits_per_sample == 16 ? 2 : 1) bytes per pixel. */
int mic_hip_wsi_format(const uint8_t *compressed, size_t compressed_len, int *channels, int *bits_per_sample, int *color_transform);
/* ReadWSIHeader (wsicompress.go:299). */
int mic_hip_wsi_info(const uint8_t *compressed, size_t compressed_len, int *width, int *height,
                     int *tile_w, int *tile_h, int *levels, uint64_t *total_tiles);
int mic_hip_wsi_level_info(const uint8_t *compressed, size_t compressed_len, int level,
                           int *width, int *height, int *tiles_x, int *tiles_y);
/* Replaces DecompressWSITile (wsicompress.go:175): one tile, cropped at the level's edge;
 * *out_w x *out_h pixels are written (3 bytes each for RGB, 1 or 2 for greyscale). */
int mic_hip_wsi_decompress_tile(const uint8_t *compressed, size_t compressed_len, int level, int tile_x, int tile_y,
                                uint8_t *rgb_out, size_t out_cap, int *out_w, int *out_h);
/* All tiles of one pyramid level in a single batch, stitched into a level-sized image. */
int mic_hip_wsi_decompress_level(const uint8_t *compressed, size_t compressed_len, int level,
                                 uint8_t *rgb_out, size_t out_cap);
/* DecompressWSIRegion(data, level, x, y, w, h) (wsicompress.go:219-297): a rectangle of one pyramid level; w and h are
 * clamped to the level as the reference does and returned through out_w / out_h (may be NULL). */
int mic_hip_wsi_decompress_region(const uint8_t *compressed, size_t compressed_len, int level,
                                  int x, int y, int w, int h,
                                  uint8_t *rgb_out, size_t out_cap, int *out_w, int *out_h);

/* Many patches per call, into a tensor that already lives on the device (no reference counterpart; beside
 * mic_hip_wsi_decompress_region, which serves one rectangle through the host).  Patch i is the rectangle [xy[2i], xy[2i] + pw) x
 * [xy[2i + 1], xy[2i + 1] + ph) of pyramid level `level`; coordinates may be negative and the rectangle may overhang the level:
 * pixels outside the level are 0 (_decompress_region clamps instead; a batch needs one shape).  The union of the tiles the
 * patches touch is decoded, each tile once, in slabs of the unit codec's sub-batch size, and a kernel writes each patch-tile
 * overlap (a "piece") from the decoded planes straight into d_out: n x ph x pw x channels samples, patch-major, row-major,
 * interleaved, in the slide's sample format (u8 RGB; u8 or little-endian u16 greyscale), n * ph * pw * bytes-per-pixel bytes, every
 * one of them written.  d_out is memory the device can write: a device allocation on the call's device or pinned host memory
 * (mic_hip_host_alloc); anything else is MIC_ERR_ARGS, found with hipPointerGetAttributes before anything is launched.
 * status[i] (host, may be NULL): MIC_OK, or the first non-OK status among patch i's tiles in tile-index order -- the code
 * mic_hip_wsi_decompress_tile returns for that tile; such a patch's pixels are unspecified, every other patch is exact.
 * Returns MIC_OK when the call ran, even if patches failed; n == 0 is MIC_OK; MIC_ERR_ARGS for level, pw, ph <= 0 or n < 0,
 * MIC_ERR_CAPACITY for out_cap below the tensor's size, MIC_ERR_UNSUPPORTED / MIC_ERR_CORRUPT for the header (a tile index entry
 * that points outside the file counts as the header's).  One device: the calling thread's default session (the file and reader
 * forms) or the given session; no fan-out over mic_hip_set_devices, the output being one device tensor.
 * stats (may be NULL): tiles decoded (the union's size), pieces gathered, slabs (decode chains) the call ran. */
typedef struct { uint64_t tiles_decoded, pieces, slabs; } mic_hip_patch_stats;
/* The host planner of those calls, beside mic_hip_shard_plan and mic_hip_wsi_band_plan: the tiles (ty * tiles_x + tx of a level of
 * level_w x level_h pixels; tile sizes 0 = 256) the patches touch, ascending, each once, into tiles[cap]; *ntiles their number,
 * *npieces the number of patch-tile overlaps with non-empty area (both may be NULL).  More than cap tiles: MIC_ERR_CAPACITY with
 * the counts set and tiles untouched.  Needs no device. */
int mic_hip_wsi_patch_plan(int level_w, int level_h, int tile_w, int tile_h, const int32_t *xy, int n, int pw, int ph,
                           uint64_t *tiles, size_t cap, uint64_t *ntiles, uint64_t *npieces);
int mic_hip_wsi_read_patches(const uint8_t *compressed, size_t compressed_len, int level, const int32_t *xy, int n, int pw, int ph,
                             void *d_out, size_t out_cap, int32_t *status, mic_hip_patch_stats *stats);

/* Patches of many slides and levels per call (no reference counterpart; what mic_hip_strips_read_crops is to strip files).  The
 * text of "Many patches per call" above carries over except as stated here.  Patch i = xysl[4i .. 4i + 3] = (x, y, slide, level) is
 * the rectangle [x, x + pw) x [y, y + ph) of pyramid level `level` of files[slide] (readers[slide]); origins may be negative, a
 * patch may overhang its level or lie wholly outside it, samples outside the level are 0.  d_out receives n x ph x pw x channels
 * samples, every byte written; it is a device allocation on the call's device or pinned host memory, judged before anything is
 * launched (and 2-byte aligned for 16-bit samples, else MIC_ERR_ARGS).
 * The caller states the call's ONE sample format: channels / bits_per_sample = 3/8, 1/8 or 1/16.  In this order, before a file is
 * looked at: MIC_ERR_ARGS for pw, ph <= 0, n < 0, nfiles < 0 or a NULL array that is needed (xysl with n > 0; files, lens or readers
 * with nfiles > 0); MIC_ERR_UNSUPPORTED for any other format pair; MIC_ERR_CAPACITY for out_cap below the tensor's size.  Then
 * MIC_ERR_ARGS for a slide index outside [0, nfiles); n == 0 is MIC_OK with zeroed stats; d_out == NULL is MIC_ERR_ARGS.
 * A slide fails alone: a NULL pointer or reader (MIC_ERR_ARGS), a header that is refused or unsupported (the header's code), a
 * sample format other than the call's (MIC_ERR_ARGS), a tile-index entry of a touched tile that points outside the file
 * (MIC_ERR_CORRUPT) give that code to status[i] of every patch of that slide, whose samples are all 0; no other slide is affected.
 * Slides no patch names are not looked at: not parsed, not read through their reader, and may be NULL.  A patch whose level is
 * outside its slide's [0, levels) gets MIC_ERR_ARGS and zeros.  Otherwise status[i] is MIC_OK or the code of the first failing tile
 * of patch i in tile-index order, as in mic_hip_wsi_decompress_tile; such a patch's samples are unspecified, every other patch is
 * exact.  Returns MIC_OK when the call ran, even if patches failed.
 * Work is the union of the touched tiles over all slides and levels, each entropy-decoded once, ordered by slide, then by global
 * tile index (level.first + ty * tiles_x + tx).  They go through the unit codec in sub-batches of at most 65535 / P tiles (P planes
 * a tile) and no more than the workspace ceiling holds of the sub-batch's largest tile; slides of different tile sizes share
 * sub-batches, a cut may fall anywhere.  Behind each sub-batch one gather launch writes its pieces into d_out.
 * stats (may be NULL): tiles_decoded and pieces are the planner's counts, slabs the number of decode chains, slides_read the
 * number of named slides whose header was accepted (format included).
 * One device: the calling thread's default session; no fan-out over mic_hip_set_devices.  There is no session-store form: a
 * session's store holds one slide. */
typedef struct { uint64_t tiles_decoded, pieces, slabs, slides_read; } mic_hip_multi_patch_stats;
/* The host planner of those calls: needs no device and reads only headers, level tables and tile indexes.  slide_of[u] / tile_of[u]
 * (cap entries each) receive the units in decode order; *ntiles_out their number, *npieces the number of patch-tile overlaps with
 * non-empty area (both may be NULL); file_status[nfiles] (may be NULL) each slide's code, MIC_OK for slides no patch names.  More
 * than cap units: MIC_ERR_CAPACITY with the counts and file_status set and the arrays untouched.  More than 2^31 - 1 pieces:
 * MIC_ERR_UNSUPPORTED. */
int mic_hip_wsi_multi_patch_plan(const uint8_t *const *files, const size_t *lens, int nfiles,
                                 const int32_t *xysl, int n, int pw, int ph, int channels, int bits_per_sample,
                                 uint32_t *slide_of, uint64_t *tile_of, size_t cap,
                                 uint64_t *ntiles_out, uint64_t *npieces, int32_t *file_status);
int mic_hip_wsi_multi_read_patches(const uint8_t *const *files, const size_t *lens, int nfiles,
                                   const int32_t *xysl, int n, int pw, int ph, int channels, int bits_per_sample,
                                   void *d_out, size_t out_cap, int32_t *status, mic_hip_multi_patch_stats *stats);

/* ---- MIC3 streaming: a row-push writer and a random-access reader ------------------------------- */
/* For slides too large for one host buffer (the reference's "WSI streaming API" roadmap item, io.ReaderAt / io.WriteSeeker).
 * pwrite-like sink: write len bytes at an absolute offset, 0 = success.  The ranges of one file never overlap.
 * pread-like source (io.ReaderAt): fill dst with exactly len bytes from offset, 0 = success.
 * A callback that returns non-zero makes the call MIC_ERR_IO. */
typedef int (*mic_hip_write_fn)(void *user, uint64_t offset, const uint8_t *data, size_t len);
typedef int (*mic_hip_read_fn)(void *user, uint64_t offset, uint8_t *dst, size_t len);
typedef struct mic_hip_wsi_writer mic_hip_wsi_writer;
typedef struct mic_hip_wsi_reader mic_hip_wsi_reader;
/* Writer.  Formats, defaults and MIC_ERR_UNSUPPORTED cases are mic_hip_wsi_compress_ex's, checked before a device is touched.
 * The sink receives the file mic_hip_wsi_compress_ex writes for the same slide, byte for byte, whatever the push schedule and
 * band_tile_rows.  The slide is coded in bands of band_tile_rows tile rows (0 = automatic: one band fills a sub-batch of the unit
 * codec, capped at 256 MiB of level-0 pixels; never a function of height).  Each level keeps its current band plus one carried row
 * on the device; one kernel per band makes every level's new rows.  Level-0 tile blobs go to the sink as soon as their band is
 * coded (the file's blobs start with level 0); blobs of levels >= 1 are held in host memory and written at finish, then the header,
 * level table and tile index at offset 0.  Host memory: the upper levels' blobs, 16 bytes per tile and one band of staging.
 * Device memory (mic_hip_wsi_writer_device_bytes, at open) depends on width, tile size, band_tile_rows and format only.
 * push_rows takes the next nrows >= 1 rows, top to bottom (width * bytes per pixel each, 16-bit samples little-endian); rows past
 * height are MIC_ERR_ARGS and consume nothing.  finish before all rows are pushed is MIC_ERR_ARGS.  A sink or device error is
 * sticky: later pushes and finish return it.  close always frees; an unfinished file is abandoned.
 * The writer owns a session on the default device (devices[0] of mic_hip_set_devices: a stream is not spread over several GPUs)
 * and holds no default-pool session between calls.  Calls on one handle are serialised; different handles may run in parallel.
 * stats: bands coded, rows of level 0 per band, device time of the band pyramid kernel summed over them (ms), peak host bytes held. */
int mic_hip_wsi_writer_open(int width, int height, int channels, int bits_per_sample, int tile_w, int tile_h, int levels,
                            int band_tile_rows, mic_hip_write_fn write, void *user, mic_hip_wsi_writer **w);
int mic_hip_wsi_writer_push_rows(mic_hip_wsi_writer *w, const uint8_t *rows, int nrows);
int mic_hip_wsi_writer_finish(mic_hip_wsi_writer *w, uint64_t *file_len);
int mic_hip_wsi_writer_device_bytes(const mic_hip_wsi_writer *w, uint64_t *bytes);
int mic_hip_wsi_writer_stats(const mic_hip_wsi_writer *w, uint64_t *bands, int *band_rows, double *pyramid_ms, uint64_t *host_bytes_peak);
void mic_hip_wsi_writer_close(mic_hip_wsi_writer *w);
/* Reader.  open reads the header, level table and tile index (48 + 20 * levels + 16 * tiles bytes) through the callback and
 * validates them as the flat-buffer calls do; open and info need no device.  Tile and region decodes read only the blobs of the
 * tiles they cover (contiguous blobs of one tile row in one read) and return the pixels mic_hip_wsi_decompress_tile / _region
 * return for the whole file.  A blob outside file_len is MIC_ERR_CORRUPT.  Calls on one handle are serialised, and so are its
 * callbacks. */
int mic_hip_wsi_reader_open(mic_hip_read_fn read, void *user, uint64_t file_len, mic_hip_wsi_reader **r);
int mic_hip_wsi_reader_info(const mic_hip_wsi_reader *r, int *width, int *height, int *tile_w, int *tile_h, int *levels,
                            int *channels, int *bits_per_sample);
int mic_hip_wsi_reader_decompress_tile(mic_hip_wsi_reader *r, int level, int tile_x, int tile_y,
                                       uint8_t *out, size_t out_cap, int *out_w, int *out_h);
int mic_hip_wsi_reader_decompress_region(mic_hip_wsi_reader *r, int level, int x, int y, int w, int h,
                                         uint8_t *out, size_t out_cap, int *out_w, int *out_h);
/* mic_hip_wsi_read_patches through the reader (beside _reader_decompress_region): the blobs of the union's tiles are pulled in one
 * pass, each once, contiguous ones in one read; nothing else of the file is read. */
int mic_hip_wsi_reader_read_patches(mic_hip_wsi_reader *r, int level, const int32_t *xy, int n, int pw, int ph,
                                    void *d_out, size_t out_cap, int32_t *status, mic_hip_patch_stats *stats);
/* mic_hip_wsi_multi_read_patches through readers (slide = an index into readers[]): each named slide's blobs are pulled in one
 * request, each once, contiguous ones in one read; a reader no patch names is never called and may be NULL.  A callback that
 * fails makes the call MIC_ERR_IO before anything is launched (d_out is then untouched).  Every distinct named reader is locked
 * once, in address order: a reader listed twice, or two threads that pass the same readers in different orders, do not deadlock. */
int mic_hip_wsi_readers_read_patches(mic_hip_wsi_reader *const *readers, int nreaders,
                                     const int32_t *xysl, int n, int pw, int ph, int channels, int bits_per_sample,
                                     void *d_out, size_t out_cap, int32_t *status, mic_hip_multi_patch_stats *stats);
void mic_hip_wsi_reader_close(mic_hip_wsi_reader *r);
/* MIC2 reader: mic_hip_mic2_read_crops on a file behind a pread-like source.  open pulls the 20-byte header and then the
 * 8 * nframes-byte frame table through the callback, and nothing else, and validates them as mic_hip_mic2_info does; open and
 * info need no device.  read_crops pulls only the blobs of the plan's frames (mic_hip_mic2_crop_plan), each once, contiguous ones in
 * one read.  Calls on one handle are serialised, and so are its callbacks. */
typedef struct mic_hip_mic2_reader mic_hip_mic2_reader;
int mic_hip_mic2_reader_open(mic_hip_read_fn read, void *user, uint64_t file_len, mic_hip_mic2_reader **r);
int mic_hip_mic2_reader_info(const mic_hip_mic2_reader *r, int *width, int *height, int *nframes, int *temporal);
int mic_hip_mic2_reader_read_crops(mic_hip_mic2_reader *r, const int32_t *xyz, int n, int cw, int ch, int cd,
                                   void *d_out, size_t out_cap, int32_t *status, mic_hip_crop_stats *stats);
void mic_hip_mic2_reader_close(mic_hip_mic2_reader *r);
/* mic_hip_mic2_multi_read_crops through readers (volume = an index into readers[]; an entry no crop names may be NULL and is not
 * read): each named reader's blobs are pulled before anything is launched, each once, neighbours in the file in one read; a failing
 * callback makes the call MIC_ERR_IO with d_out untouched.  Distinct named readers are locked once, in address order. */
int mic_hip_mic2_readers_read_crops(mic_hip_mic2_reader *const *readers, int nreaders,
                                    const int32_t *xyzv, int n, int cw, int ch, int cd, void *d_out, size_t out_cap,
                                    int32_t *status, int32_t *failed_frame, mic_hip_multi_crop_stats *stats);

/* ---- single-frame RGB and the CLI's single-frame files ------------------------------------------ */
/* Replaces CompressRGB / DecompressRGB (rgbcompress.go:25-33): YCoCg-R, then the three planes as in a WSI tile blob
 * ([Y_len][Co_len][Cg_len] u32 LE + plane blobs); width and height travel out of band, as in the reference. */
int mic_hip_rgb_compress(const uint8_t *rgb, int width, int height, uint8_t *out, size_t out_cap, size_t *out_len);
int mic_hip_rgb_decompress(const uint8_t *compressed, size_t compressed_len, int width, int height,
                           uint8_t *rgb_out, size_t out_cap);
/* MICR file (writeMICRFile, cmd/mic-compress/main.go:62-91): "MICR", width, height, CompressRGB blob. */
int mic_hip_micr_compress(const uint8_t *rgb, int width, int height, uint8_t *out, size_t out_cap, size_t *out_len);
int mic_hip_micr_info(const uint8_t *compressed, size_t compressed_len, int *width, int *height);
int mic_hip_micr_decompress(const uint8_t *compressed, size_t compressed_len, uint8_t *rgb_out, size_t out_cap);
/* Many RGB images of any sizes, one call (rgbcompress.go:25-33; compressRGBTileBlob / decompressRGBTileBlob, wsicompress.go:319-363,
 * 431-475): the reference reaches this by calling CompressRGB from many goroutines -- the frames of an ultrasound cine loop, a
 * directory of visible-light images.  A sub-batch's images come up once, one kernel runs YCoCg-R over all of them and finds every
 * plane's {min, max}, the host picks the plane modes (compressWSIPlane, :373-421), ONE unit batch codes every non-constant plane, a
 * kernel assembles the blobs and each job's bytes go down in one copy.  Through the pipeline of the other batches: sub-batches under
 * the workspace ceiling with the transfers of one overlapping the kernels of its neighbours, pinned buffers sent in place,
 * mic_hip_set_devices shards by pixels.  Every job's bytes equal mic_hip_rgb_compress's (container 0) or mic_hip_micr_compress's
 * (container 1), byte for byte.  The return value is MIC_OK when the batch ran; a job with bad arguments, a buffer too small, a
 * corrupt blob or a failing plane fails alone: status, and failed_plane = the plane the error is about (0 Y, 1 Co, 2 Cg -- the
 * reference's "Y plane: %w", :339-347, :448-460), -1 when it is not a plane's.
 * out_cap >= MIC_HIP_RGB_BOUND(width * height) (+ 12 for a MICR file) is always sufficient: three raw planes. */
#define MIC_HIP_RGB_BOUND(npx) (12 + 3 * (1 + 2 * (size_t)(npx)))
typedef struct mic_hip_rgb_enc_job {
    const uint8_t *rgb;        /* in : width*height*3 bytes, interleaved (host memory) */
    int32_t   width, height;   /* in : width * height <= 2^26 */
    int32_t   container;       /* in : 0: CompressRGB blob, 1: MICR file */
    uint8_t  *out;             /* in : caller buffer */
    size_t    out_cap;         /* in  */
    size_t    out_len;         /* out */
    int32_t   status;          /* out */
    int32_t   failed_plane;    /* out */
} mic_hip_rgb_enc_job;
typedef struct mic_hip_rgb_dec_job {
    const uint8_t *compressed; /* in : a CompressRGB blob or a MICR file (host memory) */
    size_t    compressed_len;  /* in  */
    uint8_t  *rgb_out;         /* in : width*height*3 bytes (host memory) */
    size_t    out_cap;         /* in  */
    int32_t   width, height;   /* in : blob: the image's.  MICR: 0 = take the header's, else must equal it */
    int32_t   container;       /* in : 0 / 1 as above */
    int32_t   status;          /* out */
    int32_t   failed_plane;    /* out */
} mic_hip_rgb_dec_job;
int mic_hip_rgb_compress_batch(mic_hip_rgb_enc_job *jobs, int njobs);     /* rgbcompress.go:25-27, wsicompress.go:319-363 */
int mic_hip_rgb_decompress_batch(mic_hip_rgb_dec_job *jobs, int njobs);   /* rgbcompress.go:31-33, wsicompress.go:431-475 */
/* MIC1 file (writeMicFile, cmd/mic-compress/main.go:26-59): "MIC1", width, height, pipeline = 1, payload length,
 * CompressSingleFrame{,4State,8State} stream (nstates = 2, 4 or 8; the decoder auto-detects). */
int mic_hip_mic1_compress(const uint16_t *pixels, int width, int height, uint16_t max_value, int nstates,
                          uint8_t *out, size_t out_cap, size_t *out_len);
int mic_hip_mic1_info(const uint8_t *compressed, size_t compressed_len, int *width, int *height);
int mic_hip_mic1_decompress(const uint8_t *compressed, size_t compressed_len, uint16_t *pixels_out, size_t out_cap_px);

/* ---- device-resident sessions (inputs and outputs stay in HBM) ------------------------------ */
/* A session owns the workspace for up to max_units units of up to max_px pixels each and
 * runs the same kernels as the calls above on data that is already on the device.  This is
 * what bench.py times; it is also what a caller that produces / consumes pixels on the GPU
 * should use.  All pointers named d_* are device pointers. */
typedef struct mic_hip_session mic_hip_session;

int  mic_hip_session_create(mic_hip_session **s, int max_units, size_t max_px_per_unit);   /* on the default session's device */
/* The same on an explicit HIP device: the session's stream and workspace live there, and every call on the session makes that
 * device current for the calling thread first, so one host process can own a session per GPU and drive them from any thread. */
int  mic_hip_session_create_on(int device, mic_hip_session **s, int max_units, size_t max_px_per_unit);
int  mic_hip_session_device(mic_hip_session *s);
/* Device memory the session holds (bytes).  The unit codec lays its per-unit slabs out in two tiers: tier 1 -- one token per pixel
 * and an eighth, tables for 8192 symbols: about 7 bytes per pixel + 0.2 MB per unit -- is where every batch starts; a batch in
 * which a unit would cross a tier-1 capacity (more escapes than that, a 14-bit-and-up alphabet) is run again on the worst-case
 * slabs (42 bytes per pixel + 1.7 MB) and the session stays there: *tier2 (may be NULL) says so.  Results never depend on the tier. */
size_t mic_hip_session_workspace_bytes(mic_hip_session *s, int *tier2);
void mic_hip_session_destroy(mic_hip_session *s);

typedef struct mic_hip_unit {
    uint64_t px_offset;     /* first pixel of the unit, in u16 elements from d_pixels */
    int32_t  width, height;
    uint16_t max_value;
    uint16_t nstates;       /* 2 / 4 / 8, optionally | MIC_HIP_PRED_GRAD or | MIC_HIP_GAP_REMOVAL */
} mic_hip_unit;
/* OR'ed into mic_hip_unit.nstates: the unit uses the gradient-adaptive predictor of CompressSingleFrameGrad /
 * DecompressSingleFrameGrad (multiframecompress.go:111-142, deltagradrlecompressu16.go) instead of avg(left, top).  The
 * stream does not record its predictor (PICA keeps it in the strip's flags word), so decode units must carry it too.
 * Width: like the reference, no limit of its own (a unit's pixel count is bounded as for every unit).  Up to 32768 columns the
 * decoder hands rows from band to band through LDS; wider units take the row from the output frame instead, bit for bit the
 * same pixels at a lower rate. */
#define MIC_HIP_PRED_GRAD 0x200
/* OR'ed into mic_hip_unit.nstates: the unit is a gap-removal stream (mic_hip_compress_frame_gap's bytes).  Decode units must carry it
 * too; with MIC_HIP_PRED_GRAD it is MIC_ERR_ARGS (the reference has no such codec). */
#define MIC_HIP_GAP_REMOVAL 0x800

/* Encode n units.  Compressed blobs are left in the session; *d_blobs receives the device
 * address of a packed buffer holding them back to back, h_offsets[n+1] (host) their byte
 * offsets, h_status[n] the per-unit status, h_nstates[n] (may be NULL) the flavour written.
 * Synchronous with respect to the host. */
int mic_hip_session_encode(mic_hip_session *s, const uint16_t *d_pixels,
                           const mic_hip_unit *units, int n,
                           const uint8_t **d_blobs, uint64_t *h_offsets,
                           int32_t *h_status, int32_t *h_nstates);
/* Decode n units whose compressed blobs are in d_blobs at h_offsets[i]..h_offsets[i+1];
 * pixels are written to d_pixels_out at units[i].px_offset. */
int mic_hip_session_decode(mic_hip_session *s, const uint8_t *d_blobs,
                           const uint64_t *h_offsets, const mic_hip_unit *units, int n,
                           uint16_t *d_pixels_out, int32_t *h_status);
/* Asynchronous forms used for timing: enqueue all kernels of a pass on the session's
 * stream (returned by mic_hip_session_stream as a hipStream_t) without touching the host;
 * results are fetched with the *_finish calls. */
void *mic_hip_session_stream(mic_hip_session *s);
/* The buffers a session hands out (*d_blobs, *d_streams) are reused by its next call; a caller that keeps them copies them out:
 * a device-to-device copy on the calling thread's current device, complete on return. */
int mic_hip_device_copy(void *d_dst, const void *d_src, size_t bytes);
int mic_hip_session_encode_enqueue(mic_hip_session *s, const uint16_t *d_pixels,
                                   const mic_hip_unit *units, int n);
int mic_hip_session_encode_finish(mic_hip_session *s, const uint8_t **d_blobs,
                                  uint64_t *h_offsets, int32_t *h_status, int32_t *h_nstates);
int mic_hip_session_decode_enqueue(mic_hip_session *s, const uint8_t *d_blobs,
                                   const uint64_t *h_offsets, const mic_hip_unit *units, int n,
                                   uint16_t *d_pixels_out);
int mic_hip_session_decode_finish(mic_hip_session *s, int32_t *h_status);
/* Digests and checks on device-resident units (mic_hip_verify_result and the CRC: above, "verified encode").  All three are
 * synchronous with respect to the host; PICA pair batches are not served.
 * digest: h_crc[i] = the CRC-32 of unit i's pixels at d_pixels + units[i].px_offset (max_value and nstates are not looked at).
 * verify: the streams at d_blobs + h_offsets[i] .. h_offsets[i + 1] are decoded -- units as for mic_hip_session_decode -- into a
 * scratch buffer of the session (sized to the batch's extent, counted by mic_hip_session_workspace_bytes) and compared with
 * d_pixels_ref, unit i at units[i].px_offset: h_res[i].status is MIC_OK, MIC_ERR_MISMATCH, or the decoder's status (then nothing
 * was compared: mismatches 0, first_mismatch -1); crc32 is the reference pixels' in every case.
 * encode_verified: mic_hip_session_encode -- *d_blobs, h_offsets and h_nstates are that call's, byte for byte --, then verify of
 * the packed streams against d_pixels.  A unit the encoder refused (MIC_ERR_USE_RLE, MIC_ERR_INCOMPRESSIBLE, ...) keeps that
 * status in h_res[i], is not decoded, and still gets its CRC. */
int mic_hip_session_digest(mic_hip_session *s, const uint16_t *d_pixels, const mic_hip_unit *units, int n, uint32_t *h_crc);
int mic_hip_session_verify(mic_hip_session *s, const uint8_t *d_blobs, const uint64_t *h_offsets, const mic_hip_unit *units, int n,
                           const uint16_t *d_pixels_ref, mic_hip_verify_result *h_res);
int mic_hip_session_encode_verified(mic_hip_session *s, const uint16_t *d_pixels, const mic_hip_unit *units, int n,
                                    const uint8_t **d_blobs, uint64_t *h_offsets, int32_t *h_nstates,
                                    mic_hip_verify_result *h_res);
/* WaveletV2 on device-resident frames (BASELINE config 3 as bench.py times it): nframes frames of rows x cols u16, contiguous at
 * d_frames -> their streams WITHOUT the 11-byte file header (rows u32, cols u32, maxValue u16, levels u8,
 * waveletfsecompressu16.go:346-350 -- the caller holds those), packed back to back in the session: *d_streams,
 * h_offsets[nframes + 1], h_status[nframes]; *levels_applied = the level count the header carries (:321-330).  decode is the
 * inverse for streams of one shape and level count.  Files written from these streams equal mic_hip_wavelet_v2_compress's. */
int mic_hip_session_wavelet_v2_encode(mic_hip_session *s, const uint16_t *d_frames, int nframes, int rows, int cols, int levels,
                                      const uint8_t **d_streams, uint64_t *h_offsets, int32_t *h_status, int *levels_applied);
int mic_hip_session_wavelet_v2_decode(mic_hip_session *s, const uint8_t *d_streams, const uint64_t *h_offsets, int nframes,
                                      int rows, int cols, int levels, uint16_t *d_pixels_out, int32_t *h_status);
/* decode at reduced resolution (mic_hip_wavelet_v2_decompress_level_batch): frame i's band to d_pixels_out + i * nr[level] * nc[level];
 * h_symbols_decoded (nullable): tANS symbols decoded per frame. */
int mic_hip_session_wavelet_v2_decode_level(mic_hip_session *s, const uint8_t *d_streams, const uint64_t *h_offsets, int nframes,
                                            int rows, int cols, int levels, int level, uint16_t *d_pixels_out,
                                            int32_t *h_status, uint64_t *h_symbols_decoded);
/* The same pair over frames of any shapes in ONE launch chain (mic_hip_wavelet_v2_compress_jobs on device-resident data; the caller
 * cuts lists that outgrow the workspace, mic_hip_wavelet_v2_batch_plan).  encode_mixed: frame i = h_rows_cols[2 i] x h_rows_cols[2 i + 1]
 * u16 at d_frames + h_px_offsets[i] (elements), `levels` asked of every frame; its header-less stream at *d_streams + h_offsets[i] ..
 * h_offsets[i + 1] (empty when h_status[i] != MIC_OK), h_levels_applied[i] = what its header carries.  decode_mixed: stream i of a frame
 * of h_rows_cols_levels[3 i .. 3 i + 2], wanted at h_level[i] (NULL: all 0); its nr[level] x nc[level] pixels to d_pixels_out +
 * h_out_offsets[i] (elements).  A frame refused by the argument gate fails alone. */
int mic_hip_session_wavelet_v2_encode_mixed(mic_hip_session *s, const uint16_t *d_frames, const uint64_t *h_px_offsets, const int32_t *h_rows_cols,
                                            int nframes, int levels, const uint8_t **d_streams, uint64_t *h_offsets, int32_t *h_status,
                                            int32_t *h_levels_applied);
int mic_hip_session_wavelet_v2_decode_mixed(mic_hip_session *s, const uint8_t *d_streams, const uint64_t *h_offsets, const int32_t *h_rows_cols_levels,
                                            const int32_t *h_level, int nframes, uint16_t *d_pixels_out, const uint64_t *h_out_offsets,
                                            int32_t *h_status, uint64_t *h_symbols_decoded);
/* MIC3 on a device-resident slide (BASELINE config 5 as bench.py times it).  encode = CompressWSI (wsicompress.go:27-171) up
 * to, but without, the container: pyramid, tiles, YCoCg-R, plane modes and every plane's CompressSingleFrame on the device, the
 * coded planes kept in a store the session owns (device bytes + one host record per plane); *compressed_bytes = the size of the
 * MIC3 file they make.  write = WriteMIC3 (wsiformat.go:99-165) around the store: the file mic_hip_wsi_compress_ex would have
 * written, byte for byte.  decode_level = every tile of one pyramid level, from the store, into a device image of that level
 * (width * height * channels * bytes per sample); levels = the pyramid's shape. */
int mic_hip_session_wsi_encode(mic_hip_session *s, const uint8_t *d_pixels, int width, int height, int channels, int bits_per_sample,
                               int tile_w, int tile_h, int levels, uint64_t *total_tiles, uint64_t *compressed_bytes);
int mic_hip_session_wsi_write(mic_hip_session *s, uint8_t *out, size_t out_cap, size_t *out_len);
/* The same store as the container's PAYLOAD on the device -- every tile blob in container order, put together by a kernel:
 * *d_payload (valid until the session's next wsi call), its size, and tile_lens[cap >= total tiles] (host).  What a writer that
 * gathers several GPUs' tiles moves device to device; header, level table and tile index (wsiformat.go:99-165) are its own. */
int mic_hip_session_wsi_payload(mic_hip_session *s, const uint8_t **d_payload, uint64_t *payload_bytes, uint64_t *tile_lens, size_t cap);
int mic_hip_session_wsi_decode_level(mic_hip_session *s, int level, uint8_t *d_pixels_out, size_t out_cap);
int mic_hip_session_wsi_levels(mic_hip_session *s, int *levels, int *widths, int *heights, int cap);
/* mic_hip_wsi_read_patches from the slide mic_hip_session_wsi_encode left in the session (beside _decode_level): the compressed
 * slide stays in HBM, the plane records are used as they stand -- a training loop's sampler.  d_out on the session's device. */
int mic_hip_session_wsi_read_patches(mic_hip_session *s, int level, const int32_t *xy, int n, int pw, int ph,
                                     void *d_out, size_t out_cap, int32_t *status, mic_hip_patch_stats *stats);

/* mic_hip_rgb_compress_batch / _decompress_batch on device-resident data (rgbcompress.go:25-33; wsicompress.go:319-363, 431-475):
 * image i is imgs[i].width x imgs[i].height interleaved RGB at d_rgb + imgs[i].rgb_off (any byte alignment).  encode leaves the
 * CompressRGB blobs back to back in the session -- *d_blobs, blob i at h_offsets[i] .. h_offsets[i + 1], none for an image that
 * failed -- until the session's next call (mic_hip_device_copy keeps them); decode reads blobs laid out that way and writes image
 * i's pixels to d_rgb_out + imgs[i].rgb_off.  status / failed_plane per image as in the batch jobs. */
typedef struct mic_hip_rgb_image { uint64_t rgb_off; int32_t width, height; } mic_hip_rgb_image;
int mic_hip_session_rgb_encode(mic_hip_session *s, const uint8_t *d_rgb, const mic_hip_rgb_image *imgs, int n,
                               const uint8_t **d_blobs, uint64_t *h_offsets, int32_t *status, int32_t *failed_plane);
int mic_hip_session_rgb_decode(mic_hip_session *s, const uint8_t *d_blobs, const uint64_t *h_offsets,
                               const mic_hip_rgb_image *imgs, int n, uint8_t *d_rgb_out, int32_t *status, int32_t *failed_plane);
/* mic_hip_mic2_read_crops on a MIC2 file that lies in device memory: head = the file's first 20 + 8 * nframes bytes on the host,
 * d_file = the whole file (file_len bytes) on the session's device.  The streams of the plan's frames go device to device into the
 * session's compressed-input buffer (which keeps the 64 bytes of slack the decode kernels may read past a stream's end; the
 * caller's allocation owes them nothing) -- nothing crosses PCIe.  d_out on the session's device, or pinned host memory. */
int mic_hip_session_mic2_read_crops(mic_hip_session *s, const uint8_t *head, size_t head_len,
                                    const uint8_t *d_file, size_t file_len,
                                    const int32_t *xyz, int n, int cw, int ch, int cd,
                                    void *d_out, size_t out_cap, int32_t *status, mic_hip_crop_stats *stats);
/* mic_hip_mic2_multi_read_crops on MIC2 files that lie in device memory: heads[v] (host, head_lens[v] bytes) = at least the first
 * 20 + 8 * nframes bytes of volume v -- fewer is that volume's MIC_ERR_ARGS --, d_files[v] = the whole file (lens[v] bytes) on the
 * session's device; it may be NULL when none of that volume's frames is needed.  The streams go device to device; nothing but the
 * piece and footprint lists crosses PCIe. */
int mic_hip_session_mic2_multi_read_crops(mic_hip_session *s,
                                          const uint8_t *const *heads, const size_t *head_lens,
                                          const uint8_t *const *d_files, const size_t *lens, int nfiles,
                                          const int32_t *xyzv, int n, int cw, int ch, int cd, void *d_out, size_t out_cap,
                                          int32_t *status, int32_t *failed_frame, mic_hip_multi_crop_stats *stats);

/* mic_hip_mic2_compress_batch on volumes that lie in device memory, the files staying there: volume v is read at
 * d_frames + vols[v].px_off (u16 units; every residual's predecessor is the volume's own frame before it).  *d_files receives the
 * complete MIC2 files back to back, file v -- the 20-byte header, the frame table, the streams -- at h_offsets[v] .. h_offsets[v + 1]
 * (h_offsets: n + 1 entries on the host; a failed volume has h_offsets[v + 1] == h_offsets[v]); a kernel writes the headers and
 * tables and moves the streams to their final, arbitrarily aligned offsets.  The files are valid until the session's next call;
 * mic_hip_device_copy keeps them.  h_heads (host, may be NULL) receives the first 20 + 8 * nframes bytes of every file that was
 * written, one after the other in volume order: with d_files + h_offsets[v] and the lengths they are the arguments of
 * mic_hip_session_mic2_decode and mic_hip_session_mic2_multi_read_crops.  heads_cap below the sum over the volumes whose arguments
 * were accepted is MIC_ERR_CAPACITY before anything is launched; s, vols, d_files or h_offsets NULL, n < 0, d_frames NULL with
 * n > 0: MIC_ERR_ARGS.  status / failed_frame (n entries each, may be NULL) and stats as in the host form; nothing but tables and
 * statuses crosses PCIe. */
typedef struct mic_hip_mic2_volume { uint64_t px_off; int32_t width, height, nframes; uint16_t max_value, temporal; } mic_hip_mic2_volume;
int mic_hip_session_mic2_encode(mic_hip_session *s, const uint16_t *d_frames, const mic_hip_mic2_volume *vols, int n,
                                const uint8_t **d_files, uint64_t *h_offsets /* n+1 */,
                                uint8_t *h_heads, size_t heads_cap,
                                int32_t *status, int32_t *failed_frame, mic_hip_mic2_batch_stats *stats);
/* mic_hip_mic2_decompress_batch on MIC2 files that lie in device memory, at any byte alignment: heads[v] (host, head_lens[v] bytes) =
 * at least the first 20 + 8 * nframes bytes of volume v -- fewer is that volume's MIC_ERR_ARGS --, d_files[v] = the whole file
 * (lens[v] bytes) on the session's device.  Volume v goes to d_frames_out + px_off[v] (u16 units); a volume that would end behind
 * out_cap_px is MIC_ERR_CAPACITY alone.  The streams go device to device into the session's compressed-input buffer, frames and
 * running sums are written straight to their final place. */
int mic_hip_session_mic2_decode(mic_hip_session *s, const uint8_t *const *heads, const size_t *head_lens,
                                const uint8_t *const *d_files, const size_t *lens, int n,
                                uint16_t *d_frames_out, const uint64_t *px_off, size_t out_cap_px,
                                int32_t *status, int32_t *failed_frame, mic_hip_mic2_batch_stats *stats);

/* mic_hip_strips_read_crops on strip files that lie in device memory -- a dataset kept compressed in HBM and sampled from there.
 * heads[f] (host, head_lens[f] bytes) = at least the header and strip table of file f: its first 20 + 8 * num_strips (PICS) or
 * 16 + 16 * num_strips (PICA) bytes -- fewer is that file's MIC_ERR_ARGS --; d_files[f] = the whole file (lens[f] bytes) on the
 * session's device; it may be NULL for a file none of whose strips is needed.  The streams of the plan's strips go device to device
 * into the session's compressed-input buffer (which keeps the 64 bytes of slack the decode kernels may read past a stream's end; the
 * caller's allocations owe them nothing) -- nothing but the piece list crosses PCIe.  d_out on the session's device, or pinned host
 * memory. */
int mic_hip_session_strips_read_crops(mic_hip_session *s,
                                      const uint8_t *const *heads, const size_t *head_lens,
                                      const uint8_t *const *d_files, const size_t *lens, int nfiles,
                                      const int32_t *xyf, int n, int cw, int ch,
                                      void *d_out, size_t out_cap,
                                      int32_t *status, int32_t *failed_strip, mic_hip_strip_crop_stats *stats);

/* mic_hip_rgb_read_crops on CompressRGB blobs that lie in device memory, laid out as mic_hip_session_rgb_encode leaves them and as
 * mic_hip_session_rgb_decode reads them: file f is the blob at d_blobs + h_offsets[f] .. h_offsets[f + 1] (h_offsets: nfiles + 1
 * entries on the host) of an image of imgs[f].width x imgs[f].height; imgs[f].rgb_off is ignored.  A width or height <= 0
 * (MIC_ERR_ARGS), more than 2^26 pixels (MIC_ERR_UNSUPPORTED) or h_offsets[f + 1] < h_offsets[f] (MIC_ERR_ARGS) fails the file alone,
 * as a blob the host form refuses does.  The heads of the named blobs -- three lengths and three bytes a plane -- are read by a
 * kernel and come down in one copy; the blobs of a sub-batch go device to device into the session's compressed-input buffer (which
 * keeps the 64 bytes of slack the decode kernels may read past a stream's end; the caller's allocation owes them nothing) --
 * nothing but heads, the piece list and statuses crosses PCIe.  d_out on the session's device, or pinned host memory. */
int mic_hip_session_rgb_read_crops(mic_hip_session *s, const uint8_t *d_blobs, const uint64_t *h_offsets,
                                   const mic_hip_rgb_image *imgs, int nfiles, const int32_t *xyf, int n, int cw, int ch,
                                   void *d_out, size_t out_cap, int32_t *status, int32_t *failed_plane, mic_hip_rgb_crop_stats *stats);

/* ---- typed, scaled and channel-first output of the patch and crop readers ------------------------ */
/* The fifteen readers of many rectangles per call write the file's own sample format (u16, u8, interleaved u8 RGB).  Their _as
 * twins below take the same arguments and a trailing output description, and write the tensor a model consumes from the same
 * one gather: no cast, multiply-add or permute kernel behind it (no reference counterpart).
 * The value of an output sample, which a host reference reproduces bit for bit: x = the decoded sample as float (exact: at
 * most 65535); v = fmaf(x, a, b), ONE rounding, (a, b) the pair of the sample's source and channel; with CLAMP
 * v = fminf(fmaxf(v, clamp_lo), clamp_hi); then F32 stores v, F16 and BF16 convert that f32 value round-to-nearest-even (overflow
 * to +-inf), U8 and U16 store rintf(v) (ties to even) saturated to the type's range.
 * A source is what the multi doors index: a slide, a volume, a strip file, an RGB file; 0 in the one-source doors.  naffine picks the pair:
 * 0 = (1, 0) for all (affine may be NULL), 1 = one pair, C = one per channel, nsources * C = one per (source, channel), source-major.
 * pad is the value, converted to the output type as v is but with no affine and no clamp, of every sample the native door leaves 0
 * by definition: outside the level, image or volume, rows no strip covers, rectangles of a refused or missing source, patches with a
 * bad level.  A rectangle whose unit failed stays unspecified, with the status the native door gives it.
 * With CHANNELS_FIRST the tensor is n x C x ph x pw instead of n x ph x pw x C (C = 3: RGB slides); the flag is ignored when C == 1.
 * d_out must be aligned to the output sample (2 or 4 bytes) and out_cap hold the typed tensor; the order of the checks and their
 * codes are the native door's.  spec NULL or dtype NATIVE is the native door itself: same bytes, statuses, stats and kernels.
 * MIC2 temporal volumes keep their running sums in a u16 staging tensor of the session's workspace (the tensor's shape) and one
 * convert kernel writes the typed samples at the end of the call; independent volumes of the same call gather directly. */
#define MIC_HIP_OUT_NATIVE 0   /* the door's present format; everything else in the spec must be at its default */
#define MIC_HIP_OUT_U8     1
#define MIC_HIP_OUT_U16    2
#define MIC_HIP_OUT_F16    3
#define MIC_HIP_OUT_BF16   4
#define MIC_HIP_OUT_F32    5
#define MIC_HIP_OUT_CHANNELS_FIRST 1u   /* flags: n x C x ph x pw instead of n x ph x pw x C; ignored when C == 1 */
#define MIC_HIP_OUT_CLAMP          2u   /* flags: clamp to [clamp_lo, clamp_hi] behind the affine; needs lo < hi */
typedef struct {
    int32_t dtype; uint32_t flags;
    const float *affine;   /* naffine pairs (a, b); NULL with naffine 0 = (1, 0) */
    int32_t naffine;       /* 0; 1 = one pair; C = one per channel; nsources * C = one per (source, channel) */
    float clamp_lo, clamp_hi;
    float pad;             /* the value, in the output type, of every sample the native door leaves 0 by definition */
} mic_hip_out_spec;
/* The one judgement of a spec, for a door whose sources have `channels` samples a pixel of bits_per_sample bits (8 or 16) and that
 * takes nsources sources (1: a one-source door).  MIC_ERR_ARGS for a NULL spec or sample_bytes, an unknown dtype or flag bit,
 * naffine none of 0, 1, channels, nsources * channels, a NULL affine with naffine > 0, CLAMP with clamp_lo >= clamp_hi, a
 * non-finite a, b, clamp_lo, clamp_hi or pad, and NATIVE with anything else non-default (flags, affine, naffine, clamp, pad).
 * Otherwise MIC_OK and *sample_bytes = 1, 2 or 4: the bytes of one output sample (NATIVE: the source format's).  Needs no device;
 * every _as door calls it before anything is judged that needs one. */
int mic_hip_out_spec_check(const mic_hip_out_spec *spec, int channels, int bits_per_sample, int nsources, size_t *sample_bytes);

int mic_hip_wsi_read_patches_as(const uint8_t *compressed, size_t compressed_len, int level, const int32_t *xy, int n, int pw, int ph,
                                void *d_out, size_t out_cap, int32_t *status, mic_hip_patch_stats *stats, const mic_hip_out_spec *spec);
int mic_hip_wsi_reader_read_patches_as(mic_hip_wsi_reader *r, int level, const int32_t *xy, int n, int pw, int ph,
                                       void *d_out, size_t out_cap, int32_t *status, mic_hip_patch_stats *stats, const mic_hip_out_spec *spec);
int mic_hip_session_wsi_read_patches_as(mic_hip_session *s, int level, const int32_t *xy, int n, int pw, int ph,
                                        void *d_out, size_t out_cap, int32_t *status, mic_hip_patch_stats *stats, const mic_hip_out_spec *spec);
int mic_hip_wsi_multi_read_patches_as(const uint8_t *const *files, const size_t *lens, int nfiles,
                                      const int32_t *xysl, int n, int pw, int ph, int channels, int bits_per_sample,
                                      void *d_out, size_t out_cap, int32_t *status, mic_hip_multi_patch_stats *stats,
                                      const mic_hip_out_spec *spec);
int mic_hip_wsi_readers_read_patches_as(mic_hip_wsi_reader *const *readers, int nreaders,
                                        const int32_t *xysl, int n, int pw, int ph, int channels, int bits_per_sample,
                                        void *d_out, size_t out_cap, int32_t *status, mic_hip_multi_patch_stats *stats,
                                        const mic_hip_out_spec *spec);
int mic_hip_mic2_read_crops_as(const uint8_t *compressed, size_t compressed_len,
                               const int32_t *xyz, int n, int cw, int ch, int cd,
                               void *d_out, size_t out_cap, int32_t *status, mic_hip_crop_stats *stats, const mic_hip_out_spec *spec);
int mic_hip_mic2_reader_read_crops_as(mic_hip_mic2_reader *r, const int32_t *xyz, int n, int cw, int ch, int cd,
                                      void *d_out, size_t out_cap, int32_t *status, mic_hip_crop_stats *stats, const mic_hip_out_spec *spec);
int mic_hip_session_mic2_read_crops_as(mic_hip_session *s, const uint8_t *head, size_t head_len,
                                       const uint8_t *d_file, size_t file_len,
                                       const int32_t *xyz, int n, int cw, int ch, int cd,
                                       void *d_out, size_t out_cap, int32_t *status, mic_hip_crop_stats *stats, const mic_hip_out_spec *spec);
int mic_hip_mic2_multi_read_crops_as(const uint8_t *const *files, const size_t *lens, int nfiles,
                                     const int32_t *xyzv, int n, int cw, int ch, int cd, void *d_out, size_t out_cap,
                                     int32_t *status, int32_t *failed_frame, mic_hip_multi_crop_stats *stats, const mic_hip_out_spec *spec);
int mic_hip_mic2_readers_read_crops_as(mic_hip_mic2_reader *const *readers, int nreaders,
                                       const int32_t *xyzv, int n, int cw, int ch, int cd, void *d_out, size_t out_cap,
                                       int32_t *status, int32_t *failed_frame, mic_hip_multi_crop_stats *stats, const mic_hip_out_spec *spec);
int mic_hip_session_mic2_multi_read_crops_as(mic_hip_session *s,
                                             const uint8_t *const *heads, const size_t *head_lens,
                                             const uint8_t *const *d_files, const size_t *lens, int nfiles,
                                             const int32_t *xyzv, int n, int cw, int ch, int cd, void *d_out, size_t out_cap,
                                             int32_t *status, int32_t *failed_frame, mic_hip_multi_crop_stats *stats,
                                             const mic_hip_out_spec *spec);
int mic_hip_strips_read_crops_as(const uint8_t *const *files, const size_t *lens, int nfiles,
                                 const int32_t *xyf, int n, int cw, int ch,
                                 void *d_out, size_t out_cap,
                                 int32_t *status, int32_t *failed_strip, mic_hip_strip_crop_stats *stats, const mic_hip_out_spec *spec);
int mic_hip_session_strips_read_crops_as(mic_hip_session *s,
                                         const uint8_t *const *heads, const size_t *head_lens,
                                         const uint8_t *const *d_files, const size_t *lens, int nfiles,
                                         const int32_t *xyf, int n, int cw, int ch,
                                         void *d_out, size_t out_cap,
                                         int32_t *status, int32_t *failed_strip, mic_hip_strip_crop_stats *stats,
                                         const mic_hip_out_spec *spec);
/* RGB files: channels = 3, 8 bits, nsources = nfiles; CHANNELS_FIRST gives n x 3 x ch x cw */
int mic_hip_rgb_read_crops_as(const mic_hip_rgb_file *files, int nfiles, const int32_t *xyf, int n, int cw, int ch,
                              void *d_out, size_t out_cap, int32_t *status, int32_t *failed_plane, mic_hip_rgb_crop_stats *stats,
                              const mic_hip_out_spec *spec);
int mic_hip_session_rgb_read_crops_as(mic_hip_session *s, const uint8_t *d_blobs, const uint64_t *h_offsets,
                                      const mic_hip_rgb_image *imgs, int nfiles, const int32_t *xyf, int n, int cw, int ch,
                                      void *d_out, size_t out_cap, int32_t *status, int32_t *failed_plane, mic_hip_rgb_crop_stats *stats,
                                      const mic_hip_out_spec *spec);

/* ---- MIC3 patches at any magnification, resampled on the device ---------------------------------- */
/* The pyramid stores powers of two of the scanner's resolution; a sampler asks for a target resolution (0.5 um per pixel of a
 * slide scanned at 0.23).  The five MIC3 patch readers each have a _scaled twin below: the arguments of the _as form and a
 * trailing scale_num, scale_den -- an output pixel is scale_num / scale_den level pixels wide and high -- so that the tensor a
 * model consumes still comes out of the one call (no reference counterpart).
 * One scale per call, reduced by its gcd at the door; behind that 1 <= den <= num, num <= 16 * den and num <= 1024, anything else is
 * MIC_ERR_ARGS.  Slides that differ by a power of two in resolution meet at one scale through the per-patch level of the multi
 * doors; a scale per slide, and magnification (a scale below 1), are out of scope.
 * The value, exact in integers, which a host reference reproduces bit for bit.  Patch i at (x, y) of its level has pw x ph output
 * pixels.  In units of 1 / den of a level pixel, measured from the patch origin, output pixel (j, r) covers [j * num, (j + 1) * num)
 * x [r * num, (r + 1) * num) and level pixel (x + k, y + l) covers [k * den, (k + 1) * den) x [l * den, (l + 1) * den); wx(j, k)
 * and wy(r, l) are the lengths of the two overlaps (0 .. den); p(., c) is the decoded sample of channel c -- of an RGB slide the R,
 * G or B byte behind the YCoCg-R inverse --, 0 outside the level.  Per channel
 *     S = sum_l wy(r, l) * sum_k wx(j, k) * p(x + k, y + l, c),    v = (S + num^2 / 2) / num^2    (integer division: half rounds up).
 * At 2 / 1 that is (a + b + c + d + 2) / 4, the rule the pyramid is built by: a scaled read at 2 / 1 from level L at even origins
 * equals the native read from level L + 1 wherever that level came from whole 2 x 2 blocks.
 * v is the sample in the slide's own format, which the native spec (spec NULL or dtype NATIVE) writes; a typed spec applies the rule of
 * mic_hip_out_spec to x = v, unchanged.  pad (0 in the native format) goes to every output sample whose footprint lies wholly outside
 * the level, and to all samples of a patch the native door would zero (a refused slide, a bad level); a footprint partly outside
 * is averaged over the zero-extended level, with no renormalisation.
 * The source rectangle of a patch is sw x sh = ceil(pw * num / den) x ceil(ph * num / den) level pixels at (x, y)
 * (mic_hip_wsi_scaled_extent).  status[i]: the first failing tile among the tiles that rectangle touches, in tile-index order, with
 * the native door's codes; stats counts that plan's tiles and pieces -- feed mic_hip_wsi_patch_plan, mic_hip_wsi_multi_patch_plan and
 * mic_hip_tile_cache_plan with sw x sh.
 * How it runs: the door's own native call reads the n source rectangles into a staging tensor of native samples in the session's
 * workspace (at most a quarter of the workspace ceiling), and one resample kernel writes every sample of d_out.  Attached tile
 * caches work as they do in the native call.  Patches whose staging tensor does not fit go as consecutive groups, each one native
 * call and one resample launch: stats.slabs sums over the groups, tiles_decoded and pieces stay the whole call's plan counts (with
 * a tile cache attached tiles_decoded is what the groups really decoded).
 * The checks come in the native door's order with the scale judged right behind pw, ph and n; a scale of 1 / 1 (6 / 6) is the
 * _as door itself: same bytes, statuses, stats and kernels, no staging. */
/* The one judgement of a scale, and the source extent of a pw x ph patch under it.  MIC_ERR_ARGS for pw, ph, num or den <= 0 and
 * for a scale outside the limits above; MIC_ERR_UNSUPPORTED where (pw + 1) * num or (ph + 1) * num (reduced) passes 2^31 - 1.  sw, sh
 * may be NULL.  Needs no device. */
int mic_hip_wsi_scaled_extent(int pw, int ph, int scale_num, int scale_den, int *sw, int *sh);
int mic_hip_wsi_read_patches_scaled(const uint8_t *compressed, size_t compressed_len, int level, const int32_t *xy, int n, int pw, int ph,
                                    void *d_out, size_t out_cap, int32_t *status, mic_hip_patch_stats *stats, const mic_hip_out_spec *spec,
                                    int scale_num, int scale_den);
int mic_hip_wsi_reader_read_patches_scaled(mic_hip_wsi_reader *r, int level, const int32_t *xy, int n, int pw, int ph,
                                           void *d_out, size_t out_cap, int32_t *status, mic_hip_patch_stats *stats, const mic_hip_out_spec *spec,
                                           int scale_num, int scale_den);
int mic_hip_session_wsi_read_patches_scaled(mic_hip_session *s, int level, const int32_t *xy, int n, int pw, int ph,
                                            void *d_out, size_t out_cap, int32_t *status, mic_hip_patch_stats *stats, const mic_hip_out_spec *spec,
                                            int scale_num, int scale_den);
int mic_hip_wsi_multi_read_patches_scaled(const uint8_t *const *files, const size_t *lens, int nfiles,
                                          const int32_t *xysl, int n, int pw, int ph, int channels, int bits_per_sample,
                                          void *d_out, size_t out_cap, int32_t *status, mic_hip_multi_patch_stats *stats,
                                          const mic_hip_out_spec *spec, int scale_num, int scale_den);
int mic_hip_wsi_readers_read_patches_scaled(mic_hip_wsi_reader *const *readers, int nreaders,
                                            const int32_t *xysl, int n, int pw, int ph, int channels, int bits_per_sample,
                                            void *d_out, size_t out_cap, int32_t *status, mic_hip_multi_patch_stats *stats,
                                            const mic_hip_out_spec *spec, int scale_num, int scale_den);

/* Enables (1) / disables (0) per-kernel HIP-event timing of the enqueue calls. */
int mic_hip_session_set_timing(mic_hip_session *s, int enabled);
/* Per-kernel device time (ms, HIP events on the session stream) of the last enqueue:
 * names[i] / ms[i], returns the number of entries written (<= cap). */
int mic_hip_session_last_timings(mic_hip_session *s, const char **names, float *ms, int cap);

/* ---- MIC3: a cache of decoded tiles in device memory --------------------------------------------- */
/* A sampler draws patches of the same slides call after call, and every patch call entropy-decodes the tiles it touches.  A
 * tile cache keeps decoded tiles on the device: a reader or a session that has one attached decodes only the tiles that are not
 * resident, pulls only their blobs through the callback, and gathers hits and fresh tiles alike out of the cache.  It serves
 * mic_hip_wsi_reader_read_patches, mic_hip_session_wsi_read_patches, mic_hip_wsi_readers_read_patches and their _as twins; the
 * flat-file doors and _reader_decompress_tile / _region never use it, and a caller who attaches none runs the code it ran before.
 *
 * A cache has nslots slots for tiles of one format (tile size, channels, bits per sample; the format checks are
 * mic_hip_wsi_compress_ex's, tile_w / tile_h 0 = 256).  A slot holds one tile as pixels of the slide's sample format -- tile_w x
 * tile_h x channels samples of u8, or u16 for 16-bit greyscale, the YCoCg-R inverse already done -- padded to a multiple of 256
 * bytes: mic_hip_tile_cache_slot_bytes.  nslots = 0 is a valid cache that keeps nothing.  create, set_cache, clear, destroy,
 * get_stats and plan need no device: the arena (nslots * slot_bytes, one allocation) is made by the first patch call that uses the
 * cache, on that call's session's device; if that allocation fails the call returns its code and the cache stays empty.  A later
 * call whose session is on another device runs without the cache, each of its tiles counted as bypassed.
 *
 * An entry's key is (owner, global tile index = level.first + ty * tiles_x + tx, as mic_hip_wsi_multi_patch_plan counts).  An
 * owner is a reader, or one store generation of a session: two readers of one file are two owners, and every
 * mic_hip_session_wsi_encode drops the session's old entries.
 *
 * Replacement.  Each call that uses the cache gets the next call number.  (1) The call's tiles are walked in plan order (slide,
 * then global tile index); a resident one is a hit and is stamped with the call number.  (2) Each miss, in plan order, takes the
 * lowest-numbered free slot; else the entry with the smallest stamp below the call's number, ties to the lowest slot, which is
 * evicted; else -- every slot is stamped by this call -- the tile is bypassed: decoded into the session's slab and gathered
 * from there.  (3) A tile whose decode reports a status is released when the call has its statuses: a failed tile is never
 * resident (it counts as bypassed).  (4) A call that returns an error undoes everything: no entry added, none evicted, stamps and
 * counters as before.  mic_hip_tile_cache_plan runs this policy alone, on the host, over a trace -- the same code.
 *
 * Locking.  One mutex per cache, held by a call from its planning to its final stream synchronise: threads that share a cache
 * SERIALISE on it.  Lock order: readers first, in address order, then caches in address order.
 *
 * With a cache attached the stats of a patch call read: tiles_decoded = tiles this call entropy-decoded (misses + bypassed);
 * pieces = the planner's count; slabs = decode chains run, 0 for a call that only hit. */
typedef struct mic_hip_tile_cache mic_hip_tile_cache;
/* slots: as given at create; resident: entries now; hits, misses (decoded and kept), bypassed (decoded and not kept), evictions,
 * calls: cumulative; device_bytes: 0 until the arena is allocated */
typedef struct { uint64_t slots, resident, hits, misses, bypassed, evictions, calls, device_bytes; } mic_hip_tile_cache_stats;
int mic_hip_tile_cache_slot_bytes(int tile_w, int tile_h, int channels, int bits_per_sample, uint64_t *bytes);
int mic_hip_tile_cache_create(int tile_w, int tile_h, int channels, int bits_per_sample, uint64_t nslots, mic_hip_tile_cache **c);
/* drops every entry; owners stay attached.  NULL: MIC_OK */
int mic_hip_tile_cache_clear(mic_hip_tile_cache *c);
int mic_hip_tile_cache_get_stats(const mic_hip_tile_cache *c, mic_hip_tile_cache_stats *st);
/* MIC_ERR_ARGS, and nothing freed, while a reader or session is attached.  NULL: MIC_OK */
int mic_hip_tile_cache_destroy(mic_hip_tile_cache *c);
/* c = NULL detaches and drops the reader's entries; a slide whose tile size or sample format is not the cache's: MIC_ERR_ARGS;
 * the cache the reader already has: nothing happens.  mic_hip_wsi_reader_close detaches. */
int mic_hip_wsi_reader_set_cache(mic_hip_wsi_reader *r, mic_hip_tile_cache *c);
/* resident[i] = 1 when global tile index tiles[i] of this owner is resident, else 0; changes no state */
int mic_hip_wsi_reader_cache_probe(mic_hip_wsi_reader *r, const uint64_t *tiles, size_t n, uint8_t *resident);
/* the cache then serves mic_hip_session_wsi_read_patches{,_as}; the format is checked against the store when there is one, and
 * by each mic_hip_session_wsi_encode (a store of another format detaches the cache).  mic_hip_session_destroy detaches. */
int mic_hip_session_set_tile_cache(mic_hip_session *s, mic_hip_tile_cache *c);
int mic_hip_session_tile_cache_probe(mic_hip_session *s, const uint64_t *tiles, size_t n, uint8_t *resident);
/* The policy over a trace: keys = the calls' keys back to back (each call's distinct and ascending), call_len[k] = the length of
 * call k; outcome[i] = 0 hit, 1 miss (kept), 2 bypassed; *evictions = their total (may be NULL). */
int mic_hip_tile_cache_plan(uint64_t nslots, const uint64_t *keys, const uint32_t *call_len, int ncalls,
                            uint8_t *outcome, uint64_t *evictions);

/* ---- MIC2: a cache of reconstructed frames in device memory -------------------------------------- */
/* A 3-D sampler returns to the same volumes for a whole epoch, and every crop call of a reader entropy-decodes every frame its
 * crops overlap -- for a temporal file every frame from 0 up to the last one a crop needs.  A frame cache is the tile cache above
 * with slots of one frame each: width x height u16 samples, padded to a multiple of 256 bytes
 * (mic_hip_frame_cache_slot_bytes).  mic_hip_frame_cache_create returns the same object type, so _clear, _get_stats, _destroy,
 * mic_hip_tile_cache_plan and mic_hip_tile_cache_stats serve it unchanged; its limits are the crop doors' (sides > 0, at most
 * 2^28 pixels), nslots = 0 keeps nothing, and no device is needed before the first call that uses it.
 *
 * It serves mic_hip_mic2_reader_read_crops{,_as} and mic_hip_mic2_readers_read_crops{,_as}: readers of one call may share a cache
 * or hold different ones, and a reader without one is decoded inside the same call and keeps nothing.  The host-memory doors
 * (mic_hip_mic2_read_crops, _multi_read_crops) and the session doors keep no identity between calls and never use a cache; a
 * call none of whose readers has a cache runs the code it ran before.
 *
 * A slot always holds the RECONSTRUCTED frame, for independent and temporal files alike; the key is (owner, frame), each reader
 * an owner of its own.  A call's keys are the frames some crop overlaps, ascending, reader after reader in the order of the
 * readers' array (a reader listed twice once) -- for a temporal file the named frames themselves, not 0 .. last.  The policy
 * is the tile cache's.  Independent files: only misses and bypassed frames are fetched through the callback and decoded.
 * Temporal files: a resident frame is a key frame.  For a named frame f that is not a hit the anchor is the largest frame a < f
 * resident for this owner once the call is planned -- a hit, an earlier miss of this call, or an entry no crop named -- and only
 * the residual streams of frames a + 1 .. f are fetched and decoded (an interval several named frames share, once); with no
 * resident frame below f the chain starts at frame 0's spatial stream.  Frames in between that no crop names are summed through
 * and not stored.  The crops are gathered from whole frames, so a typed tensor needs no staging.
 *
 * Failure.  A frame whose decode reports a status is never resident, nor is any frame whose chain passes a failed residual
 * (they count as bypassed); crops that depend on one get its code and failed_frame = the failing frame, as without a cache.  A
 * call that returns an error (a failing callback, an allocation) leaves entries, stamps and counters as they were.
 *
 * Stats with a cache in the call: frames_decoded = the streams this call entropy-decoded; slabs = decode chains run, 0 for a
 * call that only hit. */
int mic_hip_frame_cache_slot_bytes(int width, int height, uint64_t *bytes);
int mic_hip_frame_cache_create(int width, int height, uint64_t nslots, mic_hip_tile_cache **c);
/* c = NULL detaches and drops the reader's entries; a cache whose format is not (the file's width, height, 1 channel, 16 bits):
 * MIC_ERR_ARGS; the cache the reader already has: nothing happens.  mic_hip_mic2_reader_close detaches. */
int mic_hip_mic2_reader_set_cache(mic_hip_mic2_reader *r, mic_hip_tile_cache *c);
/* resident[i] = 1 when frame frames[i] of this reader is resident, else 0; changes no state */
int mic_hip_mic2_reader_cache_probe(mic_hip_mic2_reader *r, const uint32_t *frames, size_t n, uint8_t *resident);
/* The reader doors run on a default session, which has no handle to time.  enabled != 0: every mic_hip_mic2_reader_read_crops{,_as}
 * of this reader then times its kernels as mic_hip_session_set_timing(s, 2) does on the session it runs on, summed over the call's
 * launch chains, and _last_timings returns the last call's entries as mic_hip_session_last_timings does (names[i] / ms[i], the
 * number written).  The frame kernel of a cached temporal call is the entry k_mic2_accumulate_frames. */
int mic_hip_mic2_reader_set_timing(mic_hip_mic2_reader *r, int enabled);
int mic_hip_mic2_reader_last_timings(mic_hip_mic2_reader *r, const char **names, float *ms, int cap);

#ifdef __cplusplus
}
#endif
#endif /* MIC_HIP_H */
