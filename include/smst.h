/* smst.h -- C ABI of the MI355X (gfx950) implementation of the Signalsmith Stretch spectral hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.  Library: libsmst_hip.so.
 *
 * Two groups of entry points:
 *
 *  (1) single-stream handle API -- one-to-one with the flat ABI the reference itself ships for its WASM
 *      build (reference: web/emscripten/main.cpp:15-77, 17 functions over a global singleton; here the
 *      singleton becomes a handle) plus the three members that ABI lacks (outputSeek/exact: reference
 *      signalsmith-stretch.h:173-207,468-491; setFreqMap in table form: :120-122).  Sample buffers are HOST
 *      pointers, planar (`buffers[channel][index]`, reference README.md:46).
 *
 *  (2) batch API -- S independent streams that share one configuration, processed together on one GPU.
 *      This is the data-parallel axis the reference does not have (one SignalsmithStretch instance per
 *      stream, signalsmith-stretch.h:34-35); each stream behaves exactly like one reference instance.
 *      Buffers are planar with explicit strides: sample (s, c, i) at base[s*streamStride + c*channelStride + i].
 *      `memory` selects SMST_MEM_HOST (staged through the library's own device buffers) or SMST_MEM_DEVICE
 *      (pointers are device pointers on the batch's GPU; the call is asynchronous on the batch's stream
 *      except for one 64-byte-per-stream readback inside process -- use smst_batch_synchronize()).
 *      Device inputs must be COMPLETE when the call is made, or the producing stream must be handed to
 *      smst_batch_wait_for_stream() first; inputs / outputs must stay valid until smst_batch_synchronize() returns (or
 *      until a stream passed to smst_batch_signal_stream() has caught up); the
 *      host-side part of a call (silence gate, block scheduler) overlaps the kernels of the previous call.
 *
 *  (3) pool API -- an EXTENSION the reference does not have: single-stream handles register with a pool, process() is split into a
 *      "begin" and an "end", and everything pending runs as ONE batched device submission per geometry.  See the section below.
 *
 * Limits the reference does not have (signalsmith-stretch.h:71-94 accepts any channel count and block size); configure / create
 * return SMST_ERR_INVALID with the limit in smst_last_error() beyond them:
 *   - 1 ... 16 channels per stream (the recurrence kernels size their per-lane channel arrays at compile time: 1-2 channels and 3-8 channels
 *     keep the per-bin records in LDS, 9-16 channels take the un-fused kernel pair with records through HBM -- slower, the same arithmetic);
 *   - fftSamples/2 = 2^k * {1, 3, 5} bands (the reference's own fast sizes: {1, 2, 3, 4, 5, 6, 8} * 2^k), at most 16384 (the largest
 *     of them below 19200: one FFT buffer of bands*8 bytes has to fit a CU's LDS).  Up to 9600 bands (every preset up to 96 kHz: presetDefault there has 6144) both ping-pong buffers do; beyond that --
 *     the presets at 176.4 / 192 kHz: 10240 / 12288 bands -- the second buffer lives in memory (slower per frame, the same arithmetic);
 *   - vertical step of the phase prediction, round(fftSamples/interval), at most 62 (interval >= fftSamples/62: it has to fit the
 *     wavefront's skew) with 1-4 channels, at most 30 with 5-9 channels and at most 14 with 10-16 channels (the un-fused recurrence
 *     keeps a history ring of a power of two >= step + 2 bins per channel in a CU's LDS); interval <= block.
 *   - Sample = float arithmetic only (the C++ drop-in accepts double buffers and converts at the boundary).
 *
 * Hardware queues: a call is pipelined over three HIP streams; in a process with streams of its own (an RCCL communicator is
 * enough) set GPU_MAX_HW_QUEUES=8 before the HIP runtime starts, or two of them may share a queue and run in submission order
 * (measured: +12 % per step).
 *
 * Every function returns 0 on success and a negative code on failure (the reference has no error channel:
 * signalsmith-stretch.h is UB when unconfigured; only exact() reports, :471-480).  smst_last_error()
 * returns the message of the last failure on the calling thread.
 */
#ifndef SMST_H
#define SMST_H

#ifdef __cplusplus
extern "C" {
#endif

#define SMST_OK 0
#define SMST_ERR_INVALID (-1)  /* bad argument / unconfigured handle */
#define SMST_ERR_DEVICE (-2)   /* HIP runtime error (no GPU, out of memory, launch failure) */
#define SMST_ERR_SHORT (-3)    /* exact(): input shorter than outputSeekLength (signalsmith-stretch.h:471-480) */

/* creation flags (smst_batch_create_ex / smst_batch_create_preset_ex) */
#define SMST_FLAG_HALF_STATE 1u /* BASELINE config 5 "fp16 internal": the state that outlives a tile -- Band.output (as half2),
                                 * Prediction.energy (as the half of its square root) and the overlap-add partial sums (as half) -- is
                                 * STORED in fp16; every computation stays fp32.  The reference has no such mode (Sample is float or
                                 * double, signalsmith-stretch.h:34): results agree with it in the magnitude domain to ~1e-3 and are
                                 * no longer bit-identical across different chunkings of the same audio. */

#define SMST_MEM_HOST 0
#define SMST_MEM_DEVICE 1

const char *smst_last_error(void);
/* version of the reference API this library mirrors: {1,3,2} (signalsmith-stretch.h:36) */
void smst_reference_version(int out[3]);
int smst_device_count(void);

/* ---------------------------------------------------------------------------------------------------------
 * (1) single-stream handle API
 * ------------------------------------------------------------------------------------------------------- */
typedef struct smst_stretch smst_stretch;

/* SignalsmithStretch() / SignalsmithStretch(long seed): signalsmith-stretch.h:38-39.  device = HIP ordinal.
 * seed: the reference seeds its std::default_random_engine with it (:39, :616) and draws the per-bin time factors of stretches beyond
 * 2x from that engine (:639-640).  This library carries the same engine -- libstdc++'s (minstd_rand0 through
 * uniform_real_distribution<float>), i.e. the one a g++ build of the reference has -- so an instance created with seed S makes the
 * draws a reference instance constructed with S makes.  Stream s of a batch is the instance of seed + s. */
int smst_create(smst_stretch **out, long seed, int device);
void smst_destroy(smst_stretch *h);
/* The reference object is a plain struct and therefore COPYABLE (signalsmith-stretch.h:34-35; e.g. a std::vector of them):
 * a new handle with the configuration, every parameter and the complete processing state of `src` (input history,
 * Band.input/.prevInput/.output, Prediction.energy, overlap-add ring, scheduler state) -- both continue identically from
 * here, independently of each other.  An unconfigured `src` gives an unconfigured copy. */
int smst_clone(smst_stretch **out, const smst_stretch *src);
/* The device new single-stream objects of the C++ drop-in header are created on (the reference has no such notion): the
 * environment variable SMST_DEVICE at first use, 0 if unset, or whatever smst_set_default_device() was given last.
 * An SMST_DEVICE that is not an ordinal this process can see (not a number, or >= smst_device_count()) is an ERROR, not device 0: the
 * function reports it on stderr once and returns -1 from then on, and smst_create(..., -1) fails with SMST_ERR_INVALID and a message
 * that names the value and the device count (one rank per GPU: a silent fall-back would put every rank on GPU 0). */
int smst_default_device(void);
int smst_set_default_device(int device);

/* presetDefault / presetCheaper / configure: signalsmith-stretch.h:63-94; web/emscripten/main.cpp:43-51.
 * split: 0/1, or -1 for the preset's own default (false for default, true for cheaper). */
int smst_preset_default(smst_stretch *h, int channels, float sampleRate, int split);
int smst_preset_cheaper(smst_stretch *h, int channels, float sampleRate, int split);
int smst_configure(smst_stretch *h, int channels, int blockSamples, int intervalSamples, int split);

/* queries: signalsmith-stretch.h:42-47,96-104,166-168,205-207; main.cpp:28-39 */
int smst_block_samples(const smst_stretch *h);
int smst_interval_samples(const smst_stretch *h);
int smst_input_latency(const smst_stretch *h);
int smst_output_latency(const smst_stretch *h);
int smst_split_computation(const smst_stretch *h);
/* Number of processing steps of the newest block (blockProcess.steps, signalsmith-stretch.h:284-318: analysis, spectral processing and
 * synthesis steps as the reference counts them for this block's flags and channel count); 0 before the first block.  The C++ drop-in
 * header reports it through the reference's SIGNALSMITH_STRETCH_PROFILE_PROCESS_STEP(step, steps) hook (:329-331). */
int smst_block_steps(const smst_stretch *h);
/* Number of blocks that BEGAN in the most recent smst_process() call (the `blockProcess.samplesSinceLast >= interval` branch,
 * signalsmith-stretch.h:281, taken that many times); 0 for a call that only emitted samples of a block already under way.  The drop-in
 * header announces steps through the reference's profiling hooks only for calls in which a block began. */
int smst_blocks_started(const smst_stretch *h);
int smst_seek_length(const smst_stretch *h);
int smst_output_seek_length(const smst_stretch *h, float playbackRate);

/* reset: signalsmith-stretch.h:49-60; main.cpp:40-42 */
int smst_reset(smst_stretch *h);

/* parameters: signalsmith-stretch.h:107-135; main.cpp:52-66.  Frequencies are relative to the sample rate. */
int smst_set_transpose_factor(smst_stretch *h, float multiplier, float tonalityLimit);
int smst_set_transpose_semitones(smst_stretch *h, float semitones, float tonalityLimit);
int smst_set_formant_factor(smst_stretch *h, float multiplier, int compensatePitch);
int smst_set_formant_semitones(smst_stretch *h, float semitones, int compensatePitch);
int smst_set_formant_base(smst_stretch *h, float baseFreq);
/* setFreqMap (signalsmith-stretch.h:120-122) in table form: table[i] = map((i + 0.5)/(2n)), linear in between
 * and beyond; n = 0 removes the map.  In a batch every stream keeps its own table, knot for knot, whatever the lengths of
 * the other streams' tables (no call on one stream changes another stream's map). */
int smst_set_freq_map_table(smst_stretch *h, const float *table, int n);

/* seek / process / flush: signalsmith-stretch.h:140-165, 210-423, 427-464; main.cpp:68-76 */
int smst_seek(smst_stretch *h, const float *const *inputs, int inputSamples, double playbackRate);
int smst_process(smst_stretch *h, const float *const *inputs, int inputSamples, float *const *outputs, int outputSamples);
int smst_flush(smst_stretch *h, float *const *outputs, int outputSamples, float playbackRate);
/* outputSeek / exact: signalsmith-stretch.h:173-204, 468-491 */
int smst_output_seek(smst_stretch *h, const float *const *inputs, int inputLength);
int smst_exact(smst_stretch *h, const float *const *inputs, int inputSamples, float *const *outputs, int outputSamples);

/* ---------------------------------------------------------------------------------------------------------
 * (3) pool API -- EXTENSION: nothing in this section exists in the reference
 *
 * The reference's calling pattern -- one object per stream, process() in a loop -- costs one device round trip per object and call (two
 * PCIe copies, ~60 launches, two synchronisations for ONE stream's work).  A synchronous per-object process() cannot be pooled behind the
 * caller's back; this section makes the pooling explicit.  Handles are attached to a pool; smst_process_begin() records a request and
 * returns; smst_pool_run() (or the first smst_process_end() that finds its request still pending) runs EVERYTHING pending: the members are
 * grouped by (channels, block, interval, split), each group is one batch engine whose streams are the members' slots (the slot count grows
 * geometrically, slots of detached members are reused), and a run issues exactly ONE engine call per group that has pending requests --
 * each member with its own sample counts, members without a request masked out -- through the pool's own pinned staging: one gather of
 * the members' planes, one host-to-device copy, one copy back, one scatter.  Steady-state runs allocate nothing.
 *
 * Identity: a member's output is bit for bit what the same handle, unattached, produces for the same sequence of calls, whatever the other
 * members do -- seeded random time factors beyond 2x included.  Attaching, detaching, a regrowth of the group and the destruction of the
 * pool in the middle of a stream change nothing in what follows.
 *
 * Program order per object: at most ONE request is pending per handle.  These calls on a member whose request is pending first run the
 * pool, then act: a second smst_process_begin, smst_process, every setter, seek, flush, output_seek, exact, reset, configure / presets,
 * smst_clone, smst_destroy, smst_block_steps, smst_blocks_started.  configure moves the member to its new geometry's group.  Every call of
 * section (1) works unchanged on a member and is synchronous as ever; it runs on the member's slot alone.  A clone of a member is an
 * unattached, independent handle.
 *
 * LIFETIME: `inputs` / `outputs` given to smst_process_begin -- the pointer arrays AND the planes they point to -- must stay valid and
 * untouched until the request has run (smst_process_end on that handle, or a smst_pool_run, has returned).
 *
 * Threading: a pool and its members are used from one thread at a time, as a reference object is.
 * ------------------------------------------------------------------------------------------------------- */
typedef struct smst_pool smst_pool;
int smst_pool_create(smst_pool **out, int device);
/* runs what is pending, then detaches every member: the members stay valid handles and keep their state */
void smst_pool_destroy(smst_pool *p);
/* configured or not; the handle must live on the pool's device and not be attached already (SMST_ERR_INVALID) */
int smst_pool_attach(smst_pool *p, smst_stretch *h);
/* back to an engine of its own, the state carried over (a pending request runs first) */
int smst_pool_detach(smst_stretch *h);
int smst_pool_members(const smst_pool *p);
int smst_pool_pending(const smst_pool *p);
/* everything pending: ONE engine call per geometry group.  A failure is reported here and by smst_process_end of every member it affected. */
int smst_pool_run(smst_pool *p);
/* On a member: records the request (SMST_ERR_INVALID for an unconfigured handle, negative counts, or null buffers with a non-zero count).
 * On an unattached handle: smst_process itself, so code written for the extension runs without a pool. */
int smst_process_begin(smst_stretch *h, const float *const *inputs, int inputSamples, float *const *outputs, int outputSamples);
/* Runs the pool if h's request is still pending; returns the status of h's newest request (unattached: what smst_process_begin returned). */
int smst_process_end(smst_stretch *h);
/* test hooks: engine calls issued by runs since the pool was created; device / pinned allocations and engine (re)constructions of the
 * pool -- the latter must stand still across steady-state runs */
long long smst_pool_debug_engine_calls(const smst_pool *p);
long long smst_pool_debug_allocation_events(const smst_pool *p);

/* ---------------------------------------------------------------------------------------------------------
 * (2) batch API
 * ------------------------------------------------------------------------------------------------------- */
typedef struct smst_batch smst_batch;

int smst_batch_create(smst_batch **out, int streams, int channels, int blockSamples, int intervalSamples,
                      int split, int device, long seed);
/* preset: 0 = presetDefault (block = 0.12 sr, interval = 0.03 sr), 1 = presetCheaper (0.1 sr, 0.04 sr) */
int smst_batch_create_preset(smst_batch **out, int streams, int channels, int preset, float sampleRate,
                             int split, int device, long seed);
int smst_batch_create_ex(smst_batch **out, int streams, int channels, int blockSamples, int intervalSamples,
                         int split, int device, long seed, unsigned flags);
int smst_batch_create_preset_ex(smst_batch **out, int streams, int channels, int preset, float sampleRate,
                                int split, int device, long seed, unsigned flags);
void smst_batch_destroy(smst_batch *b);

int smst_batch_streams(const smst_batch *b);
int smst_batch_channels(const smst_batch *b);
int smst_batch_block_samples(const smst_batch *b);
int smst_batch_interval_samples(const smst_batch *b);
int smst_batch_fft_samples(const smst_batch *b);
int smst_batch_bands(const smst_batch *b);
int smst_batch_input_latency(const smst_batch *b);
int smst_batch_output_latency(const smst_batch *b);
int smst_batch_seek_length(const smst_batch *b);
int smst_batch_half_state(const smst_batch *b); /* 1 if created with SMST_FLAG_HALF_STATE */
int smst_batch_output_seek_length(const smst_batch *b, float playbackRate);
long long smst_batch_workspace_bytes(const smst_batch *b);

int smst_batch_reset(smst_batch *b);
/* stream = -1 applies to every stream */
int smst_batch_set_transpose_factor(smst_batch *b, int stream, float multiplier, float tonalityLimit);
int smst_batch_set_transpose_semitones(smst_batch *b, int stream, float semitones, float tonalityLimit);
int smst_batch_set_formant_factor(smst_batch *b, int stream, float multiplier, int compensatePitch);
int smst_batch_set_formant_semitones(smst_batch *b, int stream, float semitones, int compensatePitch);
int smst_batch_set_formant_base(smst_batch *b, int stream, float baseFreq);
int smst_batch_set_freq_map_table(smst_batch *b, int stream, const float *table, int n);

/* inSamples / outSamples / rates / lengths: HOST arrays with one entry per stream. */
int smst_batch_seek(smst_batch *b, const float *in, long long inStreamStride, long long inChannelStride,
                    const int *inSamples, const double *playbackRates, int memory);
int smst_batch_process(smst_batch *b, const float *in, long long inStreamStride, long long inChannelStride,
                       const int *inSamples, float *out, long long outStreamStride, long long outChannelStride,
                       const int *outSamples, int memory);
/* flush(): per stream as signalsmith-stretch.h:427-464 (the stream's output ring is read out and the stream starts afresh).  A NEGATIVE
 * outSamples[s] leaves stream s out of the call altogether -- a count of 0 still resets it, as flush(outputs, 0) of an instance does. */
int smst_batch_flush(smst_batch *b, float *out, long long outStreamStride, long long outChannelStride,
                     const int *outSamples, const float *playbackRates, int memory);
int smst_batch_output_seek(smst_batch *b, const float *in, long long inStreamStride, long long inChannelStride,
                           const int *inputLengths, int memory);
/* ---- whole clips (EXTENSION: the reference has exact() per instance, signalsmith-stretch.h:468-491; here S clips of S lengths and S rates are ONE call) ----
 * exact() of every stream: stream s is a fresh run of instance seed+s over its whole clip -- inSamples[s] input samples become exactly
 * outSamples[s] output samples, rate_s = inSamples[s]/float(outSamples[s]) -- and, as exact() of an instance, starts from reset(): the
 * stream's parameters and its random engine stay as earlier calls left them.  Per stream, in the reference's arithmetic (the one smst_exact uses):
 *   seekLength = outputSeekLength(rate_s); inSamples[s] < seekLength: the stream is TOO SHORT -- its outSamples[s] output samples are written
 *   as zeros (the PCM code of 0.0), status[s] = SMST_ERR_SHORT, and its state is untouched (the reference returns before outputSeek, :471-480);
 *   else outputSeek(in[0, seekLength)), outputIndex = int(outSamples[s] - seekLength/rate_s), process(in[seekLength, inSamples[s]) -> out[0, outputIndex)),
 *   flush(out[outputIndex, outSamples[s]), rate_s), and status[s] = SMST_OK.
 * A NEGATIVE outSamples[s] leaves stream s out of the call altogether, as the flush rule does: state, output and status[s] untouched.
 * SMST_ERR_INVALID with a message, before anything runs: outSamples[s] == 0 (the reference divides by it), a negative inSamples[s] on a
 * participating stream, a null buffer with a non-zero count, an unknown memory kind.  The call returns SMST_OK when it ran: short streams are
 * reported through `status` only.  status (may be null): [streams] host ints.  Everything written lies inside [0, outSamples[s]) of a
 * participating stream.
 * The engine runs ONE outputSeek, ONE main process and ONE flush whatever the spread of rates: two copy kernels (csrc/smst_clip.h) move each
 * stream's segments between the caller's buffers and planar images of the library's own in which every stream's stage begins at one column
 * (allocated by the first call, part of smst_batch_workspace_bytes; a second call of the same shapes allocates nothing).
 * SMST_MEM_HOST: returns with the output in place.  SMST_MEM_DEVICE: the contract of the other device-memory calls -- smst_batch_wait_for_stream
 * before, buffers alive and untouched until smst_batch_synchronize or a signalled stream has caught up; the copy kernels are ordered as the
 * conversions of the _pcm calls are ("Ordering contract" below), and no host synchronisation is added to those outputSeek, seek and flush have.
 * (They come earlier than in smst_batch_output_seek: resetting only the streams that take part uploads a mask, which waits for the batch's stream --
 * and with it for the producer handed to smst_batch_wait_for_stream -- before the first stage is enqueued.)
 * The _pcm form takes frames (formats, strides, alignment and overs as in the _pcm calls below; also SMST_ERR_INVALID: an unknown format,
 * frameStride < channels); the zeros of a short stream count as no overs. */
int smst_batch_exact(smst_batch *b, const float *in, long long inStreamStride, long long inChannelStride, const int *inSamples,
                     float *out, long long outStreamStride, long long outChannelStride, const int *outSamples,
                     int *status, int memory);
int smst_batch_exact_pcm(smst_batch *b, const void *in, long long inStreamStride, long long inFrameStride, const int *inSamples,
                         void *out, long long outStreamStride, long long outFrameStride, const int *outSamples,
                         int *status, int format, int memory);
/* ---- interleaved PCM (EXTENSION: the reference's process() is templated on its buffers, so a caller there can hand it an adaptor over an
 * interleaved frame buffer; here the conversion is part of the call and runs on the GPU) ----
 * The four calls above with FRAME buffers: sample (s, i, c) at base[s*streamStride + i*frameStride + c], strides in ELEMENTS of the
 * format, frameStride >= channels; the pointers need the element's alignment only (2 bytes for int16, ONE byte for packed int24, whose
 * strides count elements of 3 bytes), no stride need be a multiple of 16 bytes.  `format` holds for the input and the output of a call; counts, rates and lengths are as in the planar calls (frames per
 * stream; flush_pcm keeps the negative-count rule).
 *   SMST_PCM_S16  in: float(v)/32768 (exact).  out: q = roundf(v*32768), ties away from zero, clamped to [-32768, 32767]; no dither by
 *                 default -- the rule the CLI writes WAV files with --, TPDF dither as an option ("Dither" below).  NaN gives 0 (the CLI
 *                 has no such case: a NaN there ends as -32768).
 *   SMST_PCM_F32  copied bit for bit.
 *   SMST_PCM_S24  3 bytes per sample, little-endian two's complement, packed without padding (a WAV file's 24-bit data chunk).
 *                 in: float(v)/8388608 (exact).  out: roundf(v*8388608), ties away from zero, clamped to [-8388608, 8388607]; NaN gives 0.
 *                 Dither as for SMST_PCM_S16.
 *   SMST_PCM_S32  in: the int32 converted to float32 (round to nearest even: the engine is fp32, codes above 2^24 lose their low bits)
 *                 times 2^-31.  out: roundf(v*2^31) clamped to [-2^31, 2^31 - 1] -- a product at or above 2^31 gives 2147483647 --; NaN gives 0.
 *   SMST_PCM_F16  IEEE binary16.  in: widened exactly.  out: round to nearest even, subnormal halves kept, magnitudes of 65520 and above
 *                 +-inf, NaN stays NaN (numpy's float32 -> float16).
 *   (3 and 7 are no formats.)
 * The engine still works on a planar fp32 image of the call, now the library's own: a conversion kernel in front of the call and one behind it.
 * SMST_MEM_HOST: each stream's frames are gathered into pinned memory (one memcpy per stream; a frameStride > channels is gathered frame by
 *   frame), cross PCIe as ONE copy per direction -- half the bytes of the planar call for int16 and float16, 3/4 for int24 --, and the call returns with the output in place.
 * SMST_MEM_DEVICE: the kernels read / write the caller's device pointers; the call is asynchronous exactly as smst_batch_process is.
 * Ordering contract: the input conversion runs on the batch's stream behind everything smst_batch_wait_for_stream has ordered it after,
 *   and every reader of the call's input -- the silence gate runs on a stream of its own -- is ordered behind it by the edge
 *   smst_batch_wait_for_stream makes for a caller's producer; the output conversion runs behind the call's last emitting kernel and in front
 *   of whatever smst_batch_synchronize / smst_batch_signal_stream wait for.  No host synchronisation is added.  The caller's part is the
 *   planar calls': wait_for_stream before, buffers alive and untouched until synchronize / a signalled stream has caught up.
 * SMST_ERR_INVALID with a message: an unknown format, frameStride < channels, a null buffer with a non-zero count. */
#define SMST_PCM_S16 1 /* int16, full scale 32768 */
#define SMST_PCM_F32 2 /* float32 */
#define SMST_PCM_S24 4 /* packed 24-bit integer, full scale 8388608 */
#define SMST_PCM_S32 5 /* int32, full scale 2^31 */
#define SMST_PCM_F16 6 /* IEEE binary16 */
int smst_batch_process_pcm(smst_batch *b, const void *in, long long inStreamStride, long long inFrameStride, const int *inSamples,
                           void *out, long long outStreamStride, long long outFrameStride, const int *outSamples,
                           int format, int memory);
int smst_batch_seek_pcm(smst_batch *b, const void *in, long long inStreamStride, long long inFrameStride, const int *inSamples,
                        const double *playbackRates, int format, int memory);
int smst_batch_flush_pcm(smst_batch *b, void *out, long long outStreamStride, long long outFrameStride, const int *outSamples,
                         const float *playbackRates, int format, int memory);
int smst_batch_output_seek_pcm(smst_batch *b, const void *in, long long inStreamStride, long long inFrameStride, const int *inputLengths,
                               int format, int memory);
/* ---- Dither (EXTENSION; opt-in: a batch that never turns it on launches the kernels, writes the bytes and counts the launches it did before) ----
 * TPDF dither of the int16 and int24 output of the _pcm calls, from a counter-based, stateless noise source: the dither of an element is
 * a function of the stream's seed, the channel and the frame index alone, so it can be restated bit for bit on the host
 * (tests/dither_cases.py) and does not depend on how a stream's output is cut into calls.
 *
 * The dither signal.  All arithmetic is on unsigned 32-bit words, wrapping.
 *
 *   mix(x):  x ^= x>>16;  x *= 0x7feb352d;  x ^= x>>15;  x *= 0x846ca68b;  x ^= x>>16
 *   D        = the stream's 64-bit dither seed, as an unsigned 64-bit value
 *   h        = mix( mix(lo32(D) ^ 0x736d7374) ^ hi32(D) )              per stream (the host can precompute it)
 *   key(c)   = mix( h + 0x9E3779B9*(c + 1) )                           per channel c
 *   word(n,j)= mix( mix(key(c) ^ lo32(n)) + 0x85EBCA6B*(2*hi32(n) + j + 1) )
 *              n = the 64-bit frame index, j = 0 or 1
 *   u(n,j)   = float(word(n,j) >> 8) * 2^-24 - 0.5                     in [-0.5, 0.5), exact in fp32
 *
 * - SMST_DITHER_TPDF (1): d = u(n,0) + u(n,1).  It is white and triangular on (-1, 1) LSB.
 * - SMST_DITHER_TPDF_HP (2): d = u(n,0) - u(n-1,0), with n-1 taken modulo 2^64.  It is the same triangle with lag-1 correlation -1/2, so
 *   the noise power moves towards Nyquist.  It needs no carried state because u(n-1,0) is recomputed from the counter.
 * - SMST_DITHER_NONE (0): today's rule.
 *
 * Both sums are exact in fp32.
 *
 * Quantisation rule
 * - t = v*scale + d.  This is one fp32 rounding.  The product is a power-of-two scaling and exact, so the result is the same whether or
 *   not the compiler fuses it into a multiply-add.
 * - q = roundf(t), ties away from zero.
 * - Clamp as today.
 * - NaN gives 0 as today.
 *
 * Overs
 * - An element counts as clamped iff roundf(t) lies outside the format's range.  That is, the dithered value was clamped.
 * - nans counts as today.
 *
 * Formats
 * - Dither applies to SMST_PCM_S16 and SMST_PCM_S24 only.
 * - For S32, F16 and F32 the output is bit-identical to today whatever the mode.  fp32 has nothing below an int32 LSB, and float formats
 *   are not quantised to a fixed step.
 * - S24 near full scale has an fp32 ulp of 0.5 LSB.  The mirror reproduces this because it adds in float32.
 *
 * Known answers
 * - mix(1) = 0x688990c0.  mix(0xffffffff) = 0x6768824a.
 * - key: D = 0, c = 0: 0xd56e12bd;  D = 0, c = 1: 0x56302af1;  D = -7, c = 1: 0xdbfc9700;  D = 2^40+5, c = 15: 0xdbe9456e.
 * - word(n,0) for D=0, c=0, n=0,1,2: 0x8ea83340 0xd3f7b664 0xa82e2bc5.  word(n,1) for the same: 0x73eac46c 0xdfcaa731 0x2ea8393e.
 * - For D=0, c=0, n=0,1,2: d*2^24 = 168695, 11780701, -2697628 (TPDF) and -7219755, 4542339, -2869643 (HP).
 * - For D=-7, c=1, n = 0, 2^32-1, 2^32, 2^64-1: d*2^24 = 7581456, 5086807, 515381, 7516847 (TPDF) and 1786397, -1939039, -6678722, -988138 (HP).
 * - int16 codes of the constant v = 0.3/32768 for D=0, c=0, n=0..15:
 *     TPDF: 0 1 0 0 1 0 0 0 0 0 -1 0 0 0 0 1        HP: 0 1 0 0 0 0 1 0 0 0 0 1 0 0 0 1
 *
 * Frame index n.  Every stream has a frame counter.  In smst_batch_process_pcm and smst_batch_flush_pcm, frame i of stream s in a call has
 * n = counter_s + i, and after the call counter_s += max(outSamples[s], 0) -- for every stream whose mode is not NONE, whatever the call's
 * format.  So a stream's dithered output does not depend on how it is cut into calls, and a flush continues the sequence.  Only
 * smst_batch_set_pcm_dither resets the counter; smst_batch_reset does not.
 * In smst_batch_exact_pcm n is the output frame's index within the clip, from 0: the counter is neither read nor advanced, so the same clip
 * gives the same file.  The zeros of a too-short stream stay the code of 0.0, undithered, and count no overs; streams left out stay untouched.
 * The per-stream entries (mode, h, lo32 and hi32 of the first n) ride in the per-call table the _pcm calls upload anyway (the exact call:
 * the same table, uploaded beside its segments): no allocation and no host synchronisation is added to any call, the ordering contract is
 * unchanged, and a steady-state dithered call leaves smst_batch_debug_allocation_events where it is.
 * SMST_ERR_INVALID with a message: an unknown mode, a stream index out of range, a null batch. */
#define SMST_DITHER_NONE 0
#define SMST_DITHER_TPDF 1
#define SMST_DITHER_TPDF_HP 2
/* stream = -1: every stream, stream s getting seed + s (the batch's own seed rule); sets the stream's frame counter to 0 */
int smst_batch_set_pcm_dither(smst_batch *b, int stream, int mode, long long seed);
/* any pointer may be null; frames = the stream's frame counter */
int smst_batch_pcm_dither(const smst_batch *b, int stream, int *mode, long long *seed, long long *frames);
/* ---- Level (EXTENSION; opt-in: a batch that never calls smst_batch_set_pcm_level launches the kernels, writes the bytes and counts the launches it did before) ----
 * Per-stream output gain and peak meters in the output conversion of the _pcm calls and, for whole clips (smst_batch_exact_pcm), a gain
 * derived from the clip's own peak.  A batch uses the levelled kernels from its first smst_batch_set_pcm_level on; a stream that was never
 * set has the gain 1, and v*1 is v.
 *
 * Arithmetic.  Every step is one correctly rounded fp32 operation, so it can be restated bit for bit on the host (tests/level_cases.py).
 * - w = v*g: one fp32 multiply of its own, never fused into what follows.
 * - Then the rule of the format runs on w: t = w*scale (+ d), roundf, clamp, NaN gives 0.  The float formats (F32, F16) write w.
 * - Overs count as before, on t.  Dither is unchanged and comes after the gain.
 *
 * Peak.  The largest |v| BEFORE the gain, over the frames a call writes for the stream and over all channels.  NaNs are skipped, +-inf
 * counts as inf.  Peaks are compared as the unsigned bit patterns of |v| -- an integer maximum: order-independent, bit-reproducible.
 *
 * Modes
 * - SMST_LEVEL_FIXED (0): g = gain.  Any finite gain: 0 mutes, a negative one inverts.
 * - SMST_LEVEL_PROTECT (1), whole clips only: q = ceiling/peak, g = gain <= q ? gain : q -- the gain, lowered where the clip would exceed the ceiling.
 * - SMST_LEVEL_NORMALISE (2), whole clips only: g = ceiling/peak (the gain is not used).
 *   peak is that of the stream's whole output clip [0, outSamples[s]), q the correctly rounded fp32 quotient; peak 0 or not finite: g = gain.
 *   The peak is measured (one pass over the library's own planar image of the output) and the gain formed on the device: no host
 *   synchronisation is added to the call.  A peak so small that the quotient overflows gives g = inf, as the arithmetic says.
 *
 * Which calls.  smst_batch_process_pcm and smst_batch_flush_pcm apply the gain of FIXED streams and meter them; if a stream that takes part
 * (process: every stream; flush: those with a non-negative count) has a whole-clip mode they return SMST_ERR_INVALID before anything runs --
 * a whole-clip gain in a streaming call would be a silent lie.  smst_batch_exact_pcm serves all three modes.  The too-short and left-out
 * streams of an exact call stay as they are: undithered zeros or untouched, peak and gain unchanged.  Out of scope: the planar calls and the
 * planar smst_batch_exact are neither levelled nor metered; separate input and output formats in one call.  (The peak above is the SAMPLE
 * peak; "True peak" below has the inter-sample meter and what it does to the ceilings, "Limiter" the stage that meets a ceiling frame by
 * frame instead of lowering the whole clip's gain.)
 *
 * Clip-free ceilings.  fl(peak*fl(ceiling/peak)) may exceed the ceiling by an fp32 rounding or two, so a ceiling of exactly full scale can
 * clamp.  No element is clamped (smst_batch_take_pcm_overs gives 0) when ceiling*scale is at most
 *
 *     format   no dither      TPDF / TPDF_HP
 *     S16      32767          32766
 *     S24      8388606        8388605
 *     S32      2^31 - 256     (S32 is not dithered)
 *
 * and the next code up (S32: the next float32, 2^31 - 128) does clamp for some peak.  Found by pushing sampled peaks through a float32
 * mirror, which tests/level_cases.py repeats; the float formats have no ceiling to respect.
 *
 * The per-stream entries (mode, gain, ceiling) ride in the per-call table beside the dither entries; the meters ([3][streams] words:
 * peaks, applied gains, the clip peaks of the newest exact call) are device memory allocated with the batch and part of
 * smst_batch_workspace_bytes.  No allocation and no host synchronisation is added to any call, the ordering contract is unchanged, and a
 * steady-state levelled call leaves smst_batch_debug_allocation_events where it is.
 * SMST_ERR_INVALID with a message: an unknown mode, a stream index out of range, a null batch, a gain that is not finite, a gain <= 0 in
 * PROTECT, a ceiling that is not finite or <= 0 in the two whole-clip modes.
 *
 * Loudness.  SMST_LEVEL_LOUDNESS (3) is a third whole-clip mode, set by smst_batch_set_pcm_loudness (not by smst_batch_set_pcm_level): the
 * clip is brought to a target T in LUFS.  smst_batch_exact_pcm only; process_pcm and flush_pcm refuse it as they refuse the other two.
 * fs is the stream's loudness sample rate -- the rate of the OUTPUT clip; a parameter of the level setting, not of the engine's geometry.
 *
 * Measurement.  ITU-R BS.1770-4 integrated loudness of the stream's output clip [0, outSamples[s]), before any gain, on the library's own
 * planar image of the output.  Everything up to the final gain is float64.
 * - K-weighting: two biquads in series, coefficients computed by the host in double from fs, zero state at the clip's first sample.
 *     shelf      f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196
 *                K = tan(pi*f0/fs), Vh = 10^(G/20), Vb = Vh^0.4996667741545416, a0 = 1 + K/Q + K*K
 *                b = [(Vh + Vb*K/Q + K*K)/a0, 2*(K*K - Vh)/a0, (Vh - Vb*K/Q + K*K)/a0],  a = [1, 2*(K*K - 1)/a0, (1 - K/Q + K*K)/a0]
 *     high-pass  f0 = 38.13547087602444, Q = 0.5003270373238773, K = tan(pi*f0/fs), d = 1 + K/Q + K*K
 *                b = [1, -2, 1],  a = [1, 2*(K*K - 1)/d, (1 - K/Q + K*K)/d]
 *   Known answer: at fs = 48000 these are the standard's table -- shelf b 1.53512485958697, -2.69169618940638, 1.19839281085285; shelf a
 *   -1.69065929318241, 0.73248077421585; high-pass a -1.99004745483398, 0.99007225036621.
 * - Blocks: h = round(fs/10) samples; block i covers [i*h, i*h + 4h) of the N = outSamples[s] samples; nb = (N - 4h)/h + 1 (integer
 *   division) for N >= 4h, else 0.  z_i = sum_c w_c * (sum of y_c^2 over block i) / (4h), y_c the weighted channel c; the channel weights
 *   w_c are per batch and 1 unless set (a 5.1 caller sets 1.41 on the surrounds and 0 on the LFE).
 * - Gates, in the power domain (no logarithm is taken on the device): absolute, z_i > 10^((-70 + 0.691)/10); relative, z_i > 0.1 * the
 *   mean of the z that passed the absolute gate.  Z = the mean of the z that pass both.  The host reports L = -0.691 + 10*log10(Z).
 *   A block that holds a NaN passes no gate; a NaN poisons the filter state, so every block from the NaN's on is such a block.
 * - Loudness is undefined when nb = 0, when no block passes, or when Z is not finite or not positive (a clip of silence; one with a NaN
 *   in its first 100 ms).
 *
 * Gain.  gL = float32(sqrt(P/Z)), P = 10^((T + 0.691)/10) computed by the host in double; the division and the square root are float64
 * operations, followed by one rounding to fp32.  gL = 1 where loudness is undefined.  q = ceiling/peak exactly as PROTECT forms it from
 * the clip's peak; peak 0, a peak that is not finite or a ceiling of +inf: no limit.  g = gL <= q ? gL : q.  From there the levelled
 * conversion runs unchanged: w = v*g, the format's rule, dither after the gain.  A stream that is too short or left out stays as it is.
 *
 * How.  Four passes over the image on the device, behind the peak pass and in front of the conversion; every sum has one fixed order and
 * no floating-point atomic is used, so a call's result is bit-reproducible whatever the scheduling (csrc/smst_loudness.h).
 * The sample rate must give h >= SMST_LOUDNESS_CHUNK samples (fs >= 2555).  The per-stream entries and the channel weights ride in the
 * per-call table beside the level entries; the passes' scratch and the meters grow with the first call that measures, as the images do, and
 * count in smst_batch_workspace_bytes: a second call of the same shapes allocates nothing, no host synchronisation is added, and the
 * ordering contract of the device-memory call is unchanged.  A batch without a stream in this mode launches none of the passes.
 * Out of scope: measuring in the planar calls (momentary and short-term loudness and loudness range: "Loudness range"; the streaming frame
 * calls have a meter of their own: "Stream meter").
 * SMST_ERR_INVALID with a message: a target that is not finite; a sample rate that is not finite, <= 0 or gives h < SMST_LOUDNESS_CHUNK; a
 * ceiling <= 0 or NaN (+inf is allowed); a weight that is negative or not finite; a stream index out of range; a null batch. */
#define SMST_LEVEL_FIXED     0 /* g = gain */
#define SMST_LEVEL_PROTECT   1 /* whole clips only: q = ceiling/peak; g = gain <= q ? gain : q */
#define SMST_LEVEL_NORMALISE 2 /* whole clips only: g = ceiling/peak */
#define SMST_LEVEL_LOUDNESS  3 /* whole clips only: gL = sqrt(P/Z); g = gL <= q ? gL : q (smst_batch_set_pcm_loudness) */
#define SMST_LOUDNESS_CHUNK 256 /* frames of a clip that one lane of the loudness passes filters (kLoudChunk) */
/* stream = -1: every stream.  ceiling is checked in the two whole-clip modes only */
int smst_batch_set_pcm_level(smst_batch *b, int stream, int mode, float gain, float ceiling);
/* any pointer may be null */
int smst_batch_pcm_level(const smst_batch *b, int stream, int *mode, float *gain, float *ceiling);
/* stream = -1: every stream.  Sets the stream's mode to SMST_LEVEL_LOUDNESS (smst_batch_pcm_level then reports mode 3, gain 1 and the
 * ceiling); smst_batch_set_pcm_level takes it out of the mode again */
int smst_batch_set_pcm_loudness(smst_batch *b, int stream, double targetLufs, float ceiling, double sampleRate);
/* of a stream in SMST_LEVEL_LOUDNESS (another one: SMST_ERR_INVALID); either pointer may be null */
int smst_batch_pcm_loudness(const smst_batch *b, int stream, double *target, double *sampleRate);
/* weights: [channels], or null for 1 on every channel */
int smst_batch_set_pcm_loudness_weights(smst_batch *b, const float *weights);
/* per stream, of the newest smst_batch_exact_pcm that measured: lufs[s] = L (-inf where loudness was undefined or the stream was not
 * measured), blocks[s] = the blocks that passed the absolute gate, gated[s] = those that passed both.  Any pointer may be null.
 * Synchronises the batch.  smst_batch_take_pcm_peaks reports the gain g that was applied. */
int smst_batch_take_pcm_loudness(smst_batch *b, double *lufs, int *blocks, int *gated);
/* test hook: the four loudness passes alone on a planar fp32 image (host pointer, strides in floats) with a segment table as
 * smst_debug_clip_copy's ([streams][2][4]: a clip is segment 0 then segment 1 of its rows), per-stream sample rates ([streams]) and channel
 * weights ([channels], null: 1) -> per stream Z, the two block counts, gL for the target, and the block powers z_i
 * (blockPowers[s*maxBlocks + i], the first min(nb, maxBlocks) of them).  Any output pointer may be null. */
int smst_debug_clip_loudness(int device, int streams, int channels, const int *segments,
                             const float *image, long long imageStreamStride, long long imageChannelStride,
                             const double *sampleRates, const float *weights, double targetLufs,
                             double *Z, int *blocks, int *gated, float *gains, double *blockPowers, int maxBlocks);
/* ---- True peak (EXTENSION; opt-in: a batch that never calls smst_batch_set_pcm_true_peak launches the kernels, writes the bytes and counts the launches it did before) ----
 * Every ceiling above is a sample-peak ceiling; a delivery specification (EBU R 128, ATSC A/85) states a maximum TRUE peak, the peak of the
 * waveform between the samples as well.  A stream with the true-peak flag has the true peak of its whole output clip measured in
 * smst_batch_exact_pcm, and its whole-clip modes then form their quotient from it: the ceilings of PROTECT, NORMALISE and LOUDNESS are dBTP.
 *
 * The interpolator oversamples 4x.  The fractional phases are p = 1, 2, 3 (phase 0 is the sample itself); each has 12 taps, j = 0 ... 11:
 *     t = (j - 5) - p/4
 *     h = sinc(t) * 0.5*(1 + cos(pi*t/6))      sinc(t) = sin(pi*t)/(pi*t): a Hann window of half-width 6, |t| < 6 for every tap
 *     c[p][j] = float32(h / sum_j h)           computed by the host in double; each phase normalised to unit DC gain; one rounding
 *   Known answers: c[2] = -9.85122286e-04, 1.03496173e-02, -3.36731486e-02, 8.00664872e-02, -1.80965975e-01, 6.25208139e-01, then
 *   mirrored; c[1][5] = 8.96035254e-01, c[1][6] = 2.88544923e-01; c[3][j] = c[1][11 - j].
 *   The filter is defined by this formula, not by the 48-coefficient table of ITU-R BS.1770-4 Annex 2 (DESIGN.md states the deviation).
 *   Per-phase gain is at most 1.0118 (+0.10 dB, near 0.67 Nyquist); above 0.8 Nyquist the meter under-reads, as one of 12 taps per phase
 *   does.  A Hann-faded tone whose samples straddle its crests reads 0.99528 at fs/4 (sample peak 0.70711), 0.99930 at fs/8, 0.97687 at 3fs/8.
 *
 * Arithmetic.  Float64 up to the final comparison:
 *     y_p(n) = sum_{j = 0 ... 11} double(c[p][j]) * double(x(n + j - 5))
 *   accumulated from 0.0 in the order j = 0 ... 11, for n = 0 ... N - 1 in clip order, N = outSamples[s]; x outside [0, N) is 0.  A product
 *   of two float32 values is exact in float64, so the sum is the same with or without fused multiply-adds, and a float64 mirror that adds
 *   in the same order reproduces it bit for bit (tests/true_peak_cases.py).
 * - True peak of a stream: the maximum over channels, n and phases of the bit pattern of float32(|v|) -- v the sample x(n) itself and
 *   the three y_p(n), each rounded once to float32.  An integer maximum, as the sample peak is.  NaNs are skipped (a window that holds a
 *   NaN gives NaN), +-inf counts as inf.  The true peak is therefore >= the sample peak by construction.
 *
 * The flag is a setting of its own beside the stream's level mode: smst_batch_set_pcm_level and smst_batch_set_pcm_loudness leave it as it
 * is.  The first call with on != 0 makes the batch a levelled one, as the first smst_batch_set_pcm_level does.  In smst_batch_exact_pcm, for
 * a stream that runs:
 * - the true peak is measured (one more pass over the library's own planar image of the output, on the device);
 * - PROTECT, NORMALISE and LOUDNESS form q = ceiling/peak from the TRUE peak instead of the sample peak; everything else stays: the same
 *   correctly rounded fp32 division, the same rule for a peak of 0 or one that is not finite, the same rule for a ceiling of +inf;
 * - a FIXED stream is metered only;
 * - streams without the flag, in the same call, produce the bytes, meters and gains they produce without it.
 * The "Clip-free ceilings" table keeps holding with the flag on: the true peak is >= the sample peak, so the gain can only be lower.
 * smst_batch_take_pcm_peaks still reports the SAMPLE peak and the applied gain.
 *
 * Which calls.  smst_batch_process_pcm and smst_batch_flush_pcm return SMST_ERR_INVALID, before anything runs, if a stream that takes part
 * has the flag -- the rule and the reason of the whole-clip modes: a meter across calls would need 11 frames of carried history per channel.
 * (That meter exists as a setting of its own, with exactly that history: "Stream meter".)
 *
 * How.  One kernel (csrc/smst_true_peak.h) behind the call's last emitting kernel and in front of the conversion.  The flag rides
 * in the fourth word of the stream's level entry; the taps travel as a kernel argument.  The true-peak words ([streams] ints) are device
 * memory that grows with the first call that measures and counts in smst_batch_workspace_bytes: a second call of the same shapes allocates
 * nothing, no host synchronisation is added, and the ordering contract of the device-memory call is unchanged.  The maximum is one of
 * integers and no floating-point atomic is used: a call's result is bit-reproducible whatever the scheduling.
 * Out of scope: true-peak metering in the planar calls (the streaming frame calls: "Stream meter"); an oversampling factor that depends on the rate (4x at
 * every rate).
 * SMST_ERR_INVALID with a message: a stream index out of range, a null batch. */
#define SMST_TRUE_PEAK_TILE 1024 /* frames of a channel's clip that one workgroup of the true-peak pass measures (kTruePeakTile) */
/* stream = -1: every stream */
int smst_batch_set_pcm_true_peak(smst_batch *b, int stream, int on);
/* on may be null */
int smst_batch_pcm_true_peak(const smst_batch *b, int stream, int *on);
/* per stream, of the newest smst_batch_exact_pcm that measured: truePeaks[s] = the true peak of the stream's clip BEFORE the gain; 0 for a
 * stream that call did not measure (flag off, too short, left out) and before any call has measured.  Synchronises the batch; resets nothing. */
int smst_batch_take_pcm_true_peaks(smst_batch *b, float *truePeaks);
/* test hook: the true-peak pass alone on a planar fp32 image (host pointer, strides in floats) with a segment table as smst_debug_clip_copy's
 * ([streams][2][4]: a clip is segment 0 then segment 1 of its rows) -> per stream the true peak and, from kClipPeak on the same image, the
 * sample peak.  flags ([streams], null: every stream): the streams that have the flag; another one reports a true peak of 0.  Either output
 * pointer may be null. */
int smst_debug_clip_true_peak(int device, int streams, int channels, const int *segments,
                              const float *image, long long imageStreamStride, long long imageChannelStride,
                              float *truePeaks, float *samplePeaks, const int *flags);
/* test hook: the library's tap table c[p][j], phase-major: out[12*(p - 1) + j], p = 1, 2, 3 */
int smst_debug_true_peak_taps(float *out);
/* ---- Limiter (EXTENSION; opt-in: a batch that never calls smst_batch_set_pcm_limiter launches the kernels, writes the bytes and counts the launches it did before) ----
 * A ceiling above can only lower the gain of the WHOLE clip (g = gL <= q ? gL : q): a clip with one loud transient comes out quieter than the
 * LUFS target its caller asked for.  A stream with the limiter flag keeps its whole-clip gain and has the frames that would exceed the
 * ceiling brought down to it by a lookahead limiter, in smst_batch_exact_pcm only.  Within a stream the channels are linked: one gain curve
 * r(n).  The curve is non-recursive -- a function of the frames within 2H of n --, so it is bit-reproducible whatever the scheduling.
 *
 * The flag is a setting of its own beside the stream's level mode, as the true-peak flag is; the batch has one lookahead of H frames,
 * 1 <= H <= SMST_LIMITER_MAX_LOOKAHEAD.  The limiter acts on PROTECT and LOUDNESS streams.  FIXED has no ceiling and NORMALISE meets its
 * ceiling by construction: there the flag is inert -- r is identically 1, the call writes the bytes and launches the kernels it does without
 * the flag.  For a limited stream of N = outSamples[s] frames, x_c(n) the samples of channel c in clip order:
 * 1. g, the whole-clip gain WITHOUT the quotient q: PROTECT g = gain; LOUDNESS g = gL (1 where loudness is undefined).
 *    smst_batch_take_pcm_peaks reports this g.
 * 2. Detector: m(n) = the maximum over the channels of the bit pattern of |x_c(n)|; with the stream's true-peak flag also of
 *    float32(|y_p,c(n)|), p = 1, 2, 3 -- "True peak"'s own phases of frame n, in its float64 arithmetic, each rounded once.  NaNs are skipped.
 * 3. Need: w = m(n)*g, one fp32 multiply (|v*g| of the loudest channel: the multiply the conversion makes).  need(n) = ceiling/w, the
 *    correctly rounded fp32 quotient, where w is finite and w > ceiling; else need(n) = 1 (w not finite, a ceiling of +inf, a g that is not
 *    finite or not above 0: "no limit", as q has it).  Outside [0, N) need is 1.
 * 4. Hold: hold(i) = the minimum of need(j) over |j - i| <= H, for i in [-H, N + H).
 * 5. Smooth: win[k] = float32(h_k / sum h), h_k = 0.5*(1 + cos(pi*k/(H + 1))), k = -H ... H, computed by the host in double, one rounding.
 *    y(n) = sum_{k = -H ... H} double(win[k]) * double(hold(n + k)), in float64, from 0.0, in that order.  The products are exact, so a
 *    fused multiply-add changes nothing (the true-peak argument).
 * 6. Gain: r(n) = 1.0f exactly where every hold(n + k), |k| <= H, is 1 (no need below 1 within 2H frames); else r(n) = min(float32(y(n)),
 *    need(n)).  So r(n) <= need(n) for every frame whatever the rounding of the window, and a clip that never exceeds its ceiling gets the
 *    bytes it gets with the limiter off.
 * 7. Apply: w = v*g as in "Level", then u = w*r(n), one more fp32 multiply of its own (never fused), then the format's rule on u, dither
 *    behind it.  Overs and the sample-peak meter stay as they are.
 * The too-short and left-out streams of a call stay as they are.  smst_batch_process_pcm and smst_batch_flush_pcm return SMST_ERR_INVALID,
 * before anything runs, if a stream that takes part has the flag: the rule and the reason of the whole-clip modes.
 *   Known answers (float32 bit patterns).  Window, H = 1: 3e800000 3f000000 3e800000.  H = 2: 3daaaaab 3e800000 3eaaaaab 3e800000 3daaaaab.
 *   H = 72: win[-72] = 36d4ca98, win[-71] = 37d4b160, win[0] = 3c607038.
 *   Mono, 13 frames, x(6) = 1, else 0; g = 1, ceiling 0.5, H = 2, no true peak: r = 3f800000 3f800000 3f755556 3f555556 3f2aaaab 3f0aaaab
 *   3f000000 3f0aaaab 3f2aaaab 3f555556 3f755556 3f800000 3f800000.  5 frames, x(0) = 1, the same settings: r = 3f000000 3f0aaaab 3f2aaaab
 *   3f555556 3f755556 -- the clip's edge counts as need 1.  12 frames, x(5) = x(6) = 1, g = 1, ceiling 1, H = 1, true-peak flag on:
 *   need(5) = 3f4cbb59 (1/1.2504163: the inter-sample crest belongs to frame 5), r(3 ... 7) = 3f732ed6 3f598c83 3f4cbb59 3f598c83 3f732ed6,
 *   1 elsewhere.
 *
 * What it guarantees.  The SAMPLE peak of u is at most the ceiling, up to the fp32 roundings of ceiling/w and w*r: fl(w*fl(ceiling/w)) is the
 * function of "Clip-free ceilings" above with w in the place of the peak, and r < need only lowers it -- the same search on the limiter's
 * mirror (tests/limiter_cases.py, CPU) gives the same table: no element is clamped when ceiling*scale is at most 32767 / 32766 (int16
 * without / with dither), 8388606 / 8388605 (int24), 2^31 - 256 (int32).
 * The TRUE peak of the limited output is not bounded exactly, with or without the true-peak flag: the interpolator does not commute with a
 * gain that varies from frame to frame.  It is a measured property (the true-peak mirror on the limiter mirror's float32 output; white noise,
 * AM tones and sparse spikes driven 12 dB over the ceiling, true-peak flag on): the worst true peak exceeds the ceiling by 2.4e-6 at
 * H = 72, 2.5e-5 at H = 36, 3.4e-3 (0.03 dB) at H = 8 and 17 % (1.4 dB) at H = 1 (EXPERIMENTS.md, "Limiter").  A short lookahead weakens a dBTP promise: the window must be long against the
 * 12 taps of the interpolator.
 *
 * How.  Two kernels (csrc/smst_limiter.h) behind the peak, loudness and true-peak passes and in front of the conversion, whose
 * limited variant reads r at the frame's clip position.  The flag is bit 1 of the fourth word of the stream's level entry (bit 0: true
 * peak); H travels as a kernel argument; the window is device memory, uploaded by the setters below, never in a call.  need, r ([streams]
 * [longest limited clip] floats each) and the meter words grow with the first call that limits and count in smst_batch_workspace_bytes: a
 * second call of the same shapes allocates nothing, no host synchronisation is added, and the ordering contract of the device-memory call is
 * unchanged.  The meters are integers: no floating-point atomic.
 * Out of scope: release shaping other than the symmetric window, a lookahead per stream, oversampled gain application.  (The streaming calls
 * have a limiter of their own, a setting beside this flag: "Stream limiter" below.)
 * SMST_ERR_INVALID with a message: a lookahead outside [1, SMST_LIMITER_MAX_LOOKAHEAD], a stream index out of range, a null batch. */
#define SMST_LIMITER_MAX_LOOKAHEAD 1024
#define SMST_LIMITER_DEFAULT_LOOKAHEAD 72 /* 1.5 ms at 48 kHz */
#define SMST_LIMITER_TILE 1024 /* frames of a clip that one workgroup of either pass takes (kLimitTile) */
/* stream = -1: every stream.  The first call with on != 0 makes the batch a levelled one and puts the window into device memory */
int smst_batch_set_pcm_limiter(smst_batch *b, int stream, int on);
/* on may be null */
int smst_batch_pcm_limiter(const smst_batch *b, int stream, int *on);
/* the batch's lookahead H in frames; synchronises the batch where the window is on the device already, and clears the lines of "Stream limiter" */
int smst_batch_set_pcm_limiter_lookahead(smst_batch *b, int frames);
int smst_batch_pcm_limiter_lookahead(const smst_batch *b, int *frames);
/* per stream, of the newest smst_batch_exact_pcm that limited: minGain[s] = the lowest r(n), limitedFrames[s] = the frames with r(n) < 1;
 * 1 and 0 for a stream that call did not limit and before any call has limited.  Either may be null.  Synchronises the batch; resets nothing. */
int smst_batch_take_pcm_limiter(smst_batch *b, float *minGain, long long *limitedFrames);
/* test hook: the limiter's two passes alone on a planar fp32 image (host pointer, strides in floats) with a segment table as
 * smst_debug_clip_true_peak's.  Per stream: g = gains[s] (the PROTECT form), ceilings[s], flags[s] with bit 0 true peak and bit 1 limiter.
 * need and r: [streams][maxFrames], indexed [s*maxFrames + n], 1 where nothing is limited (maxFrames >= every clip's length); minGain,
 * limitedFrames: [streams], as smst_batch_take_pcm_limiter.  Every output pointer may be null. */
int smst_debug_clip_limit(int device, int streams, int channels, const int *segments,
                          const float *image, long long imageStreamStride, long long imageChannelStride,
                          const float *gains, const float *ceilings, const int *flags, int lookahead,
                          float *need, float *r, int maxFrames, float *minGain, long long *limitedFrames);
/* test hook: the library's window, out[k + lookahead] = win[k], k = -lookahead ... lookahead */
int smst_debug_limiter_window(int lookahead, float *out);
/* ---- Stream limiter (EXTENSION; opt-in: a batch that never calls smst_batch_set_pcm_stream_limiter launches the kernels, writes the bytes and counts the launches it did before) ----
 * The limiter above knows a whole clip.  A real-time caller who applies a gain to an int16 or int24 bus through smst_batch_process_pcm could
 * only let the conversion clamp and count the overs.  The curve of "Limiter" is non-recursive -- r(n) is a function of need over the 4H + 1
 * frames around n --, so it has an exact streaming form: with the output 2H frames late and need of the last 4H frames carried per stream,
 * a stream cut into calls in any way gets, bit for bit, the clip limiter's output.
 *
 * It is a per-stream setting of its own, on/off and a ceiling, NOT the flag above: that flag stays refused in the streaming calls.  The
 * batch's one lookahead H serves both limiters (smst_batch_set_pcm_limiter_lookahead).  The setting acts on streams in SMST_LEVEL_FIXED with
 * g = the stream's fixed gain (a stream that was never given a level: g = 1); a stream in a whole-clip mode is refused by the streaming calls
 * as ever, with the setting on as well.
 *
 * Definition.  Let v(n), n = 0, 1, 2 ..., be the frames the engine has emitted for the stream through smst_batch_process_pcm and
 * smst_batch_flush_pcm since the stream's line was last cleared.  The T frames the stream has been handed so far are the first T frames of
 * "Limiter"'s steps 2 to 7 applied to the clip [2H frames of +0.0, v(0), v(1), ... v(T - 1)], where g is the fixed gain, the detector works
 * without true-peak phases, need uses |g| -- an inverting stream is limited too; fabsf is exact, so limitNeed(m, fabsf(g), ceiling) is the
 * one definition of the step --, the ceiling is the stream limiter's own and the window is the one the batch already has.  The result does
 * not depend on how T is cut into calls, and the clip's right edge never enters: frame i < T depends on need up to i + 2H < T + 2H.
 *   Latency.  The output is the engine's, 2H frames late; smst_batch_pcm_stream_limiter_latency reports 2H.
 *   Leading frames.  The first 2H frames are the zeros in front of the stream, treated as any frame: multiplied (w = 0*g, u = w*r -- with
 *   a negative gain a float format shows -0.0), dithered with the stream's running frame counter, metered.  A loud v(0) pulls r below 1 on
 *   them, and they count as limited frames.
 *   Flush.  The line is not the engine's: a flush does not empty it.  To end a stream, its flush is asked for 2H frames more -- the
 *   reference's flush writes zeros behind its tail --, or the stream is flushed again.
 *   Meters.  The sample-peak meter and the overs stay as they are; the peak is over the |v| of the frames a call WRITES, the delayed ones.
 *   Counters.  Dither is applied behind the limiter; its frame counter advances as ever.
 *   Unflagged streams.  In the same call a stream without the setting is not delayed and gets the bytes it gets without this section; a
 *   batch may mix both.  A stream with no frame in a call, or left out of a flush, keeps its line.
 * The line is cleared (need <- 1, frames <- +0.0) by smst_batch_set_pcm_stream_limiter for the stream, on or off -- turning it off drops the
 * 2H frames inside --, by smst_batch_set_pcm_limiter_lookahead for every stream, and by smst_batch_reset.  smst_batch_set_pcm_level does NOT
 * clear it: a gain change acts on the frames whose need is formed from then on, and on every frame written from then on.
 *   Meters of its own.  minGain[s] = the lowest r written for the stream, limitedFrames[s] = the frames written with r < 1, both
 *   accumulated over the calls since the last take, which clears them as the peaks' take does.  On the device they are integer words
 *   (atomicMax, atomicAdd: no floating-point atomic); the count wraps as an unsigned 32-bit word does, the overs' rule.
 *   Known answers (float32 bit patterns).  H = 2, mono, g = 1, ceiling 0.5, 17 frames with v(6) = 1 and the rest 0, cut as 5, 1, 7, 4:
 *   r of the frames written = 3f800000 x6, 3f755556 3f555556 3f2aaaab 3f0aaaab 3f000000 3f0aaaab 3f2aaaab 3f555556 3f755556, 3f800000 x2;
 *   the float32 output is 3f000000 at frame 10 and 0 elsewhere; minGain 3f000000, limitedFrames 9.  H = 2, mono, g = -1, ceiling 0.5,
 *   9 frames with v(0) = 1, cut as 3, 6: r = 3f755556 3f555556 3f2aaaab 3f0aaaab 3f000000 3f0aaaab 3f2aaaab 3f555556 3f755556; the output
 *   is 80000000 x4, bf000000, 80000000 x4; limitedFrames 9.
 *
 *   True-peak detector.  A per-stream flag of its own beside the setting (smst_batch_set_pcm_stream_limiter_true_peak), so that a live
 *   stream meets a ceiling given in dBTP.  It is NOT smst_batch_set_pcm_true_peak, which stays refused in the streaming calls, and it is
 *   inert while the stream's setting is off.  The taps of "True peak" reach 6 frames ahead of a frame, so need of a frame exists 6 frames
 *   later: let D = 2H + 6 (SMST_STREAM_LIMITER_TRUE_PEAK_DELAY = 6).  The T frames a flagged stream has been handed so far are the first T
 *   frames of "Limiter"'s steps 2 to 7 applied to the clip [D frames of +0.0, v(0), v(1), ... v(T - 1)], where g is the fixed gain, need
 *   uses |g|, the detector is step 2 WITH the true-peak phases -- "True peak"'s own float64 sums, each rounded once, NaNs skipped --, the
 *   ceiling is the stream limiter's and the window the batch's.  Frame i < T depends on need up to i + 2H, which depends on the clip up
 *   to i + 2H + 6 < T + D: the clip's right edge never enters, the result does not depend on the cuts, and the streaming form is, bit for
 *   bit, the clip limiter with its true-peak flag on.  Everything above carries over with D in the place of 2H: the leading D zeros are
 *   treated as frames; a flush does not empty the line, and to end a stream its flush is asked for D frames more; the meters, the dither
 *   counter and the other streams of the call behave as described; the clearing rules are the same, and the flag's setter clears the
 *   stream's line as well, on or off, because the delay changes.  smst_batch_pcm_stream_limiter_latency_of reports a stream's own delay:
 *   0, 2H or 2H + 6.  Behind a stream output resample the limiter sees the delivered frames as ever; the delays add up to Dl + 2H + 6.
 *   Known answers (float32 bit patterns).  H = 2, mono, g = 1, ceiling 1, flag on, 24 frames with v(6) = v(7) = 1 and the rest 0, cut as
 *   5, 1, 7, 11 (D = 10): r of the frames written = 3f800000 x12, 3f7bba48 3f6ee91e 3f5dd23c 3f510112 3f4cbb59 3f510112 3f5dd23c 3f6ee91e
 *   3f7bba48, 3f800000 x3; the float32 output is 3f4cbb59 at frame 16 and 3f510112 at frame 17, 0 elsewhere -- the inter-sample crest
 *   belongs to v(6): need = 1/1.2504163 --; minGain 3f4cbb59, limitedFrames 9.  H = 1, mono, g = -1, ceiling 1, flag on, 12 frames with
 *   v(0) = v(1) = 1, cut as 3, 9 (D = 8): r = 3f800000 x6, 3f732ed6 3f598c83 3f4cbb59 3f598c83 3f732ed6, 3f800000; the output is 80000000
 *   x8, bf4cbb59, bf598c83, 80000000 x2; limitedFrames 5.
 *
 * What it guarantees: what the clip limiter guarantees.  The SAMPLE peak of u is at most the ceiling, up to the roundings tabulated under
 * "Clip-free ceilings" -- with the flag too: the true-peak need is never above the sample need.  The TRUE peak of a stream without the flag
 * is not bounded: on the signals of "Limiter"'s measurement (white noise, AM tones, sparse spikes, 12 dB over a ceiling of 0.5) the numpy
 * mirror's output stands 59 % over the ceiling at H = 72 and 36, 61 % at H = 8 and 67 % at H = 1.  With the flag it is the clip limiter's
 * measured property, because the outputs are the same bits: 2.4e-6 over at H = 72, 2.5e-5 at H = 36, 3.3e-3 (0.03 dB) at H = 8 and 17 %
 * at H = 1 (EXPERIMENTS.md, "Stream limiter, true-peak detector") -- a short lookahead weakens a dBTP promise here as it does there.
 *
 * How.  Per stream, in device memory and counted in smst_batch_workspace_bytes: need of the last 4H frames, the last 2H frames of every
 * channel (v, before the gain) and the meter words, allocated by the first setter call with on != 0 -- which makes the batch a levelled one
 * and puts the window on the device --, never in a call.  The lines exist twice: every kernel of a call reads one set and writes the other,
 * and everything is ordered by the batch's stream, so one pair serves calls in flight.  Three kernels (csrc/smst_stream_limiter.h):
 * need of the call's frames behind the carried ones; the curve, by the clip limiter's own steps 4 to 6 (one device function for both); and
 * a limited conversion -- a kernel of its own -- whose loader takes frame i from the line (i < 2H) or from the call's image at i - 2H.  A
 * flagged stream has a feed kernel of its own, which forms need of the c frames v(p - 6) ... v(p + c - 7) of a call of c frames after p
 * emitted ones from the 11 frames carried in front of them and the call's image, with the phases' one definition (truePeakFrameBits); it
 * carries its last 2H + 11 frames per channel -- a uniform length: the 11 of the taps and the 2H + 6 of the delay overlap in 6 --, two
 * sets again, allocated by the first call of the flag's setter with on != 0 and counted in smst_batch_workspace_bytes.  The gain pass is
 * the same launch for both kinds; a call in which no flagged stream has frames launches exactly what it launched before the flag
 * existed.  The flag is bit 4 of the level entry's fourth word.  The
 * work rows ([streams][4H + longest limited call] and [streams][longest limited call] floats) grow with the first call that needs them; a
 * steady-state call allocates nothing and no host synchronisation is added.  The setting is bit 2 of the fourth word of the stream's level
 * entry, the ceiling rides in the word a FIXED entry does not use; smst_batch_pcm_level keeps reporting the level's own ceiling.
 * Out of scope: a lookahead per stream, oversampled gain application, the planar calls, smst_batch_exact_pcm, release shaping, stretch_cli
 * (a whole-file tool, which has --limit).
 * SMST_ERR_INVALID with a message, before anything runs: a stream index out of range, a null batch, a ceiling that is NaN or <= 0 (+inf is
 * allowed: no limit); smst_batch_exact_pcm with a participating stream that has the setting on (the whole-clip form is
 * smst_batch_set_pcm_limiter). */
/* stream = -1: every stream.  Clears the line of the stream(s).  The first call with on != 0 makes the batch a levelled one, puts the window
 * into device memory and allocates the lines */
int smst_batch_set_pcm_stream_limiter(smst_batch *b, int stream, int on, float ceiling);
/* on and ceiling may be null */
int smst_batch_pcm_stream_limiter(const smst_batch *b, int stream, int *on, float *ceiling);
/* 2H: the frames by which a limited stream's output is late (a stream with the true-peak flag below: 6 more, which _latency_of reports) */
int smst_batch_pcm_stream_limiter_latency(const smst_batch *b, int *frames);
#define SMST_STREAM_LIMITER_TRUE_PEAK_DELAY 6 /* frames: what the taps of "True peak" reach ahead (kTruePeakTrail) */
/* the setting's true-peak flag ("True-peak detector" above).  stream = -1: every stream.  Clears the line of the stream(s), on or off.  The
 * first call with on != 0 allocates the lines the flag carries (and, in a batch whose setting was never on, the window and the setting's lines) */
int smst_batch_set_pcm_stream_limiter_true_peak(smst_batch *b, int stream, int on);
/* on may be null */
int smst_batch_pcm_stream_limiter_true_peak(const smst_batch *b, int stream, int *on);
/* the frames by which this stream's output is late: 0 with the setting off, 2H with it on, 2H + 6 with the flag as well.  frames may be null */
int smst_batch_pcm_stream_limiter_latency_of(const smst_batch *b, int stream, int *frames);
/* per stream, over the calls since the last take: minGain[s] = the lowest r written, limitedFrames[s] = the frames written with r < 1; 1 and
 * 0 where nothing was limited.  Either may be null.  Synchronises the batch and clears the meters. */
int smst_batch_take_pcm_stream_limiter(smst_batch *b, float *minGain, long long *limitedFrames);
/* test hook: `calls` output conversions in sequence on one device stream, with the carried lines, on a planar fp32 image (host pointer,
 * strides in floats) that holds each stream's frames in order.  counts: [calls][streams], negative = the stream takes no part in that call.
 * gains, ceilings, flags: [streams]; flags: bit 0 (1) = setting on, bit 1 (2) = the true-peak detector as well (inert without bit 0).  r: [streams][maxFrames] as written (delayed; 1 for a stream without the setting
 * and behind the frames written); frames: interleaved float32 [streams][maxFrames][channels], the F32 output (+0.0 behind the frames
 * written).  maxFrames >= the sum of every stream's counts.  minGain, limitedFrames: [streams], the meters of all the calls.  Any output
 * pointer may be null. */
int smst_debug_pcm_stream_limit(int device, int streams, int channels, int calls, const int *counts,
                                const float *image, long long imageStreamStride, long long imageChannelStride,
                                const float *gains, const float *ceilings, const int *flags, int lookahead,
                                float *r, float *frames, int maxFrames, float *minGain, long long *limitedFrames);
/* ---- Loudness range (EXTENSION; opt-in: a batch that never calls smst_batch_set_pcm_loudness_range or _caps launches the kernels, writes the bytes and counts the launches it did before) ----
 * A delivery to EBU R 128 reports the loudness range (LRA, EBU Tech 3342) and the maximum momentary and short-term loudness (EBU Tech
 * 3341) of a clip, and R 128 s1 bounds the maximum short-term loudness of short-form content.  A stream with the meter flag has all three
 * measured in smst_batch_exact_pcm, from the sums that the loudness passes form; a cap on either maximum lowers the gain of a stream in
 * SMST_LEVEL_LOUDNESS.
 *
 * Definition.  All arithmetic is float64, on the device; logarithms are taken only by the host, when it reports.  "Loudness" supplies,
 * unchanged: fs and h = round(fs/10); the channel weights w_c; the sub-block sums sub_c[j] = the sum of y_c^2 over [j*h, (j + 1)*h), j <
 * nSub, where nSub = N/h (integer division) for N >= 4h and 0 otherwise; the block powers z_i, i < nb; the absolute gate G = 10^((-70 +
 * 0.691)/10).
 * - Maximum momentary power M: the largest z_i that is not NaN, ungated; 0 when nb = 0; +inf counts.
 * - Short-term powers: ns = nSub - 29 for nSub >= 30, else 0.  For each channel q_c = sub_c[i] + ... + sub_c[i + 29], summed from 0.0 in
 *   ascending j; st_i = (sum over c, in channel order, of double(w_c)*q_c)/(30*h).
 * - Maximum short-term power ST: the largest st_i that is not NaN; 0 when ns = 0.
 * - Loudness range: absolute gate st_i > G; relative gate st_i > 0.01 * (the mean of the st that passed the absolute gate, its sum taken in
 *   block order).  n = the number that pass both (a NaN passes neither), v[0..n) those values in ascending order, kLo = ((n - 1)*10 +
 *   50)/100 and kHi = ((n - 1)*95 + 50)/100 by integer division: the nearest rank of the 10th and the 95th percentile.  The device reports
 *   lo = v[kLo], hi = v[kHi], n and ns; the host reports LRA = 10*log10(hi/lo) in LU, 0 when n = 0.
 *   The hop of 100 ms is this library's choice (Tech 3342 asks for at most 1 s); Tech 3342 itself interpolates no percentile either.
 * Known answers (a float64 restatement of the above, tests/loudness_range_cases.py): a stereo 1-kHz sine in consecutive parts of 20 s, at fs
 * = 8000 and at fs = 48000 alike --
 *     -20, -30 dBFS                     LRA 10.0000 LU   n 371   ns 371
 *     -20, -15                               5.0000         371      371
 *     -40, -20                              20.0000         371      371
 *     -50, -35, -20, -35, -50               15.0000         627      971
 *   (Tech 3342's own conformance signals; its tolerance is +-1 LU).  The maxima of the first read -19.9804 LUFS at 8 kHz and -19.9933 LUFS
 *   at 48 kHz, momentary and short-term alike.
 *
 * The meter flag is a setting of its own beside the stream's level mode, as the true-peak flag is; the first call with on != 0 makes the
 * batch a levelled one.  In smst_batch_exact_pcm a flagged stream that runs has the four loudness passes run on its output clip WHATEVER its
 * level mode, and the range stage behind them.  fs: a stream in SMST_LEVEL_LOUDNESS uses that mode's rate; any other stream the rate given
 * with the meter flag, which is checked by the rule of smst_batch_set_pcm_loudness (h >= SMST_LOUDNESS_CHUNK).  A flagged stream that is not
 * in the loudness mode gets exactly the gain its mode gives it without the flag, and smst_batch_take_pcm_loudness reports its integrated
 * loudness and counts too.  Streams without the flag, in the same call, produce the bytes, meters and gains they produce without it.
 *
 * Caps (R 128 s1).  Tm, Ts in LUFS, +inf: none.  A cap acts on SMST_LEVEL_LOUDNESS streams only, where a finite cap implies the meter;
 * elsewhere it is inert, as the limiter flag is in FIXED.  The host forms Pm = 10^((Tm + 0.691)/10) in double, Ps likewise.  The device forms
 * gm = float32(sqrt(Pm/M)) where the cap is finite and M is finite and above 0 -- division and square root in float64, one rounding --, gs
 * from Ps and ST in the same way, otherwise no cap, and gL' = min(gL, gm, gs), written over gL.  Everything that reads gL reads gL': the
 * quotient with the ceiling, the limiter's need and the conversion.  smst_batch_take_pcm_peaks reports the applied gain as before.  A stream
 * without a finite cap keeps the bits of gL.
 *
 * Which calls.  smst_batch_process_pcm and smst_batch_flush_pcm return SMST_ERR_INVALID, before anything runs, if a stream that takes part
 * has the meter flag or a finite cap: the rule of the whole-clip modes, for the same reason.  (The streaming form is a setting of its own:
 * "Stream meter".)
 *
 * How.  One kernel (csrc/smst_loudness_range.h), one workgroup per stream, behind the four loudness passes and in front of the
 * true-peak and limiter passes, launched only in a call in which a metered stream runs (launch count "clip_loudness_range"; "clip_loudness"
 * keeps counting the four passes alone).  The maxima are integer maxima; the two order statistics come from a radix select over the 64-bit
 * patterns of the gated values -- eight passes of 8 bits, integer histograms, both ranks in the same passes -- which is exact for every n and
 * reads the values where they lie, so no clip is too long for it.  No floating-point atomic is used: a call's result is bit-reproducible
 * whatever the scheduling.  The flag and the two cap powers ride in the stream's loudness entry, which now travels when any stream is
 * measured.  The short-term powers and the meter words grow with the first call that meters and count in smst_batch_workspace_bytes: a
 * second call of the same shapes allocates nothing, no host synchronisation is added, and the ordering contract of the device-memory call
 * is unchanged.
 * Out of scope: metering in the planar calls (the streaming frame calls: "Stream meter"); the time at which a maximum occurs; percentiles other than 10 and 95.
 * SMST_ERR_INVALID with a message: with on != 0, a sample rate that smst_batch_set_pcm_loudness would refuse; a cap that is NaN or -inf; a
 * stream index out of range; a null batch. */
#define SMST_LOUDNESS_RANGE_TILE 256 /* short-term powers that the range stage's workgroup takes at a time (kLoudRangeThreads) */
/* stream = -1: every stream.  sampleRate is read with on != 0 only */
int smst_batch_set_pcm_loudness_range(smst_batch *b, int stream, int on, double sampleRate);
/* the flag, and the rate last given with it (0: none yet); either pointer may be null */
int smst_batch_pcm_loudness_range(const smst_batch *b, int stream, int *on, double *sampleRate);
/* stream = -1: every stream; +inf: no cap */
int smst_batch_set_pcm_loudness_caps(smst_batch *b, int stream, double maxMomentaryLufs, double maxShortTermLufs);
int smst_batch_pcm_loudness_caps(const smst_batch *b, int stream, double *maxMomentaryLufs, double *maxShortTermLufs);
/* per stream, of the newest smst_batch_exact_pcm that metered: the two maxima in LUFS (-inf where the power is 0), range[s] = LRA in LU,
 * low[s] and high[s] = lo and hi in LUFS (-inf where n = 0), shortBlocks[s] = ns, rangeBlocks[s] = n; a stream that call did not meter, and
 * every stream before any call has metered: -inf, 0 and no blocks.  Any pointer may be null.  Synchronises the batch; resets nothing. */
int smst_batch_take_pcm_loudness_range(smst_batch *b, double *momentaryMax, double *shortTermMax, double *range,
                                       double *low, double *high, int *shortBlocks, int *rangeBlocks);
/* test hook: the four loudness passes and the range stage on a planar fp32 image; arguments as smst_debug_clip_loudness's, every stream
 * metered.  capsLufs: [streams][2] (momentary, short-term; +inf: none), null: none.  M, ST, lo and hi are reported as POWERS, gains[s] is
 * gL' of "Caps", shortPowers[s*maxBlocks + i] the first min(ns, maxBlocks) short-term powers.  Any output pointer may be null. */
int smst_debug_clip_loudness_range(int device, int streams, int channels, const int *segments,
                                   const float *image, long long imageStreamStride, long long imageChannelStride,
                                   const double *sampleRates, const float *weights, double targetLufs, const double *capsLufs,
                                   double *momentaryMax, double *shortTermMax, double *low, double *high, int *shortBlocks, int *rangeBlocks,
                                   float *gains, double *shortPowers, int maxBlocks);
/* ---- Resample (EXTENSION; opt-in: a batch that never calls smst_batch_set_pcm_resample launches the kernels, writes the bytes and counts the launches it did before) ----
 * A sample-rate converter in front of the engine, in smst_batch_exact_pcm: a stream may carry a rational ratio L/M = up/down, the batch's
 * rate over its clips' rate, and its frames are resampled on the device to the batch's rate.  Everything behind that point -- outputSeek,
 * process, flush, peak, loudness, true peak, limiter, conversion -- runs unchanged.  A caller who makes the batch's rate the delivery rate
 * gets "any rate in, one rate out"; "Output resample" below delivers each clip at a rate of its own.  The reference has no sample-rate notion beyond its presets.
 *
 * Ratio.  L and M are integers, 1 <= L, M <= SMST_RESAMPLE_MAX_TERM once the library has reduced them by their gcd; 2*M <= 9*L and 2*L <= 9*M
 * (at most 4.5 either way: 192 kHz -> 44.1 kHz is 147/640).  1/1 means "not resampled".  At most SMST_RESAMPLE_MAX_RATIOS distinct reduced
 * ratios other than 1/1 are live in a batch at a time; a ratio that no stream uses any more frees its slot.
 *
 * Lengths.  N = inSamples[s] frames at the clip's rate become Nr = ceil(N*L/M) = (N*L + M - 1)/M frames (64-bit integers; Nr must fit an
 * int).  Resampled frame n sits at input position n*M/L: i = (n*M)/L, p = (n*M) mod L, both in 64-bit integers.  Frame 0 sits on input
 * frame 0: the filter is symmetric, there is no delay.  For a resampled stream smst_batch_exact_pcm behaves exactly as if the caller had
 * handed it those Nr frames: exactLengths(Nr, outSamples[s]), rate_s = Nr/float(outSamples[s]), SMST_ERR_SHORT in status where Nr is
 * below the seek length.
 *
 * Filter: Kaiser-windowed sinc, computed by the host in double, once per ratio.  r = min(1, L/M), rho = 0.98*r, W = 32/r, H = ceil(W),
 * T = 2*H taps (64 upwards, 70 for 147/160, 128 for 1/2, 280 for 147/640).  For phase p in [0, L) and tap j in [0, T):
 * t = (j - (H - 1)) - p/L;  h = rho*sinc(rho*t)*I0(10*sqrt(1 - (t/W)^2))/I0(10) for |t| < W, else 0, sinc(x) = sin(pi*x)/(pi*x);
 * c[p][j] = float32(h / sum_j h): each phase normalised to unit DC gain, one rounding.  The filter is DEFINED by this formula, as the
 * true-peak interpolator is.  Known answers (to within one float32 ulp; bit patterns of float32):
 *   2/1:     c[0][30..32] = 3ca2f978 3f7ae0ea 3ca2f978 (0.97999442 at the centre); c[1][31] = c[1][32] = 3f22b49c (0.63556838)
 *   160/147: T = 64; c[0][31] = 3f7ae0ea; c[80][31] = c[80][32] = 3f22b49c; c[159][0] = -3.198598506e-06
 *   147/160: T = 70; c[1][34] = 3f667b0e (0.90031517), c[1][35] = 3dd53ebb; c[0][0] = 8.022285328e-06
 *   T for 1/1, 2/1, 1/2, 3/2, 2/3, 160/147, 147/160, 147/640, 640/147: 64, 64, 128, 64, 96, 64, 70, 280, 64
 * What it does (on the float32 table; 160/147, 147/160, 1/2): the passband holds within -0.053 ... +0.0001 dB up to 0.907 of the lower
 * Nyquist (20 kHz for 44.1 kHz material); everything at or above 1.093 of it -- what would alias or image into that band -- is at -100.6 dB
 * or below; in between the filter rolls off, through -11.6 dB at Nyquist.
 *
 * Arithmetic: float64, then one rounding.  y(n) = sum_{j=0...T-1} double(c[p][j])*double(x(i + j - (H - 1))), the sum from 0.0 in the order
 * j = 0 ... T-1, x outside [0, N) = 0; the resampled frame is float32(y(n)).  A product of two float32 values is exact in float64, so an FMA
 * changes nothing and a mirror that adds in the same order reproduces the device bit for bit.  x is the planar fp32 value that the
 * format's input rule gives (float(v)/32768 for int16).  Known answers, float32 bit patterns:
 *   3/2, 5 frames, x(2) = 1, Nr = 8: bca067e3 be4717b5 3ed8327b 3f7ae0ea 3ed8327b be4717b5 bca067e3 3dddb185
 *   2/3, 7 frames, x(3) = 1, Nr = 5: bc55dff0 3c594cd8 3f2740ad 3c594cd8 bc55dff0
 *   160/147, 200 frames of 1.0: Nr = 218, the frames 40 ... 169 deviate from 1 by at most 6.0e-8
 *
 * Which calls.  smst_batch_exact_pcm serves resampled streams, in host and device memory and in every format.  smst_batch_exact (planar)
 * and smst_batch_process_pcm, _seek_pcm and _output_seek_pcm return SMST_ERR_INVALID, before anything runs, if a stream that takes part has a
 * ratio other than 1/1: skipping the stage silently would be a lie.  smst_batch_flush_pcm has no input and is unaffected.  The too-short and
 * left-out streams of a call stay as they are.
 * Out of scope: resampling in the planar calls (the streaming frame calls have a setting of their own: "Stream resample" below; resampling
 * the output: "Output resample" below is the whole-clip form, "Stream output resample" the streaming one); irrational or time-varying ratios; a quality setting; a fused PCM-to-resampled kernel without the raw image.
 * SMST_ERR_INVALID with a message that names the limit: a term outside [1, SMST_RESAMPLE_MAX_TERM]; a ratio beyond 4.5 either way; a ninth
 * distinct ratio; a stream index out of range; a null batch; in a call, an Nr that does not fit an int. */
#define SMST_RESAMPLE_MAX_TERM 640
#define SMST_RESAMPLE_MAX_RATIOS 8
#define SMST_RESAMPLE_TILE 1024
/* stream = -1: every stream.  1/1 turns the stage off.  The first call with another ratio builds that ratio's table and puts it into device
 * memory: tables are never uploaded in a call */
int smst_batch_set_pcm_resample(smst_batch *b, int stream, int up, int down);
/* the stream's reduced ratio (1/1: none); either pointer may be null */
int smst_batch_pcm_resample(const smst_batch *b, int stream, int *up, int *down);
/* Nr of a clip of inSamples frames of the stream (inSamples itself at 1/1), or a negative code: what a caller derives outSamples from */
long long smst_batch_resampled_length(const smst_batch *b, int stream, long long inSamples);
/* the reduced ratio toRate/fromRate of two integer-valued rates; SMST_ERR_INVALID with a message where a rate is not a positive integer or
 * the ratio misses a limit above.  Either pointer may be null */
int smst_resample_ratio(double fromRate, double toRate, int *up, int *down);
/* test hook: the library's table of a ratio, out [L][T] phase-major (L, T of the REDUCED ratio; out may be null), *taps = T */
int smst_debug_resample_taps(int up, int down, float *out, int *taps);
/* test hook: the resample kernel alone, planar fp32 to planar fp32.  counts: [streams] N; ratios: [streams][2] up, down (1/1: the stream's
 * rows of `out` are left alone); image: each stream's clip from column 0 of its rows; segments: [streams][2][4] as smst_debug_clip_copy's,
 * the DESTINATION of the stream's Nr frames (dst and count of the two segments; the counts add up to Nr).  Host pointers, staged whole as
 * far behind a 16-byte boundary as the caller's; what the kernel leaves alone in `out` comes back as it was */
int smst_debug_clip_resample(int device, int streams, int channels, const int *counts, const int *ratios,
                             const float *image, long long imageStreamStride, long long imageChannelStride,
                             const int *segments, float *out, long long outStreamStride, long long outChannelStride);
/* ---- Output resample (EXTENSION; opt-in: a batch that never calls smst_batch_set_pcm_out_resample launches the kernels, writes the bytes and counts the launches it did before) ----
 * "Resample" brings clips of any rate to the batch's rate, and every result came back at that one rate: a caller who handed in a 44.1 kHz file
 * and wanted one back resampled the result on the CPU -- behind the loudness, true-peak, limiter and dither stages, whose figures then no
 * longer described the delivered file.  This is the converter behind the engine, in smst_batch_exact_pcm: a stream may carry a second
 * rational ratio L/M = up/down, the DELIVERY rate over the batch's rate, and the frames the engine rendered are resampled on the device
 * between the engine's output and the level stages.  The reference has no sample-rate notion beyond its presets.
 *
 * Ratio.  Per stream, reduced by the library, with the limits of "Resample": 1 <= L, M <= SMST_RESAMPLE_MAX_TERM, at most 4.5 either way;
 * 1/1 turns the stage off.  The tables are the batch's existing ratio tables -- the same formula, the same float32 table -- and the
 * SMST_RESAMPLE_MAX_RATIOS slots are shared with the other resample settings: a slot is live while any of the four settings of any stream
 * uses it.  A setter call with a ratio the batch already has allocates nothing; tables are never uploaded in a call.
 *
 * Lengths.  outSamples[s] stays what the caller receives: Nd delivered frames at the delivery rate.  The engine renders
 * E = floor((Nd - 1)*M/L) + 1 frames at the batch's rate (64-bit integers; E must fit an int): the smallest count for which the centre
 * i = (n*M)/L of every delivered frame n < Nd lies inside [0, E).  For such a stream smst_batch_exact_pcm behaves towards the engine
 * exactly as if the caller had asked for E frames: exactLengths(frames_s, E), rate_s = frames_s/float(E), where frames_s is already Nr for
 * a stream that also has the input setting; SMST_ERR_SHORT in status as ever.  The caller's buffers hold Nd frames: nothing of the call's
 * interface is sized by E (smst_batch_pcm_out_render_length reports it).
 *
 * Delivered frames.  Let r(0 ... E-1) be the rendered clip: the frames [0, outputIndex) of the main process followed by the flush.
 * Delivered frame n sits at i = (n*M)/L, p = (n*M) mod L and is float32(sum_j double(c[p][j])*double(r(i + j - (H - 1)))), j ascending
 * from 0.0, r outside [0, E) = +0.0: "Resample"'s arithmetic word for word, by the same device function.  Frames n >= Nd are not formed,
 * although ceil(E*L/M) may exceed Nd; the right edge of the filter meets zeros at E, not the frames a longer render would have held.
 * Known answers (those of "Resample"):
 *   3/2: Nd = 8 gives E = 5; r(2) = 1: bca067e3 be4717b5 3ed8327b 3f7ae0ea 3ed8327b be4717b5 bca067e3 3dddb185
 *   2/3: Nd = 5 gives E = 7; r(3) = 1: bc55dff0 3c594cd8 3f2740ad 3c594cd8 bc55dff0
 *   147/160: Nd = 441 gives E = 479 (440*160/147 = 478.9...; the 480 of "Resample"'s ceil(441*160/147) is not needed).  160/147: Nd = 480 gives E = 441.
 *
 * Everything behind the converter runs on the delivered frames: the clip peak, BS.1770 loudness and loudness range, true peak, the limiter,
 * gain, dither (whose frame index is the delivered frame's), conversion, overs and peaks.  The caller gives the DELIVERY rate as the
 * sampleRate of smst_batch_set_pcm_loudness / _loudness_range.  The limiter's lookahead stays one batch-wide count, and for such a stream
 * it counts delivered frames.  A too-short stream gets Nd zeros, as ever; a left-out stream (negative count) is untouched.
 *
 * Which calls.  smst_batch_exact_pcm serves the setting, in host and device memory and in every format, and it may be combined with
 * smst_batch_set_pcm_resample on the same stream (a 44.1 kHz file through a 48 kHz batch and back).  smst_batch_exact (planar),
 * smst_batch_process_pcm and smst_batch_flush_pcm return SMST_ERR_INVALID with a message, before anything runs, if a stream that takes part
 * has an output ratio other than 1/1.  smst_batch_seek_pcm and smst_batch_output_seek_pcm write no output and are unaffected.
 *
 * How.  The engine's output image gets a third column behind the flush's; one kernel (csrc/smst_resample_out.h) reads each such
 * stream's two-piece rendered clip and writes its delivered frames there, and the level stages and the conversion find them as one
 * segment.  Streams at 1/1 keep their two segments, and their bytes, in the same call.  The call's table of rendered segments and entries
 * exists twice, is allocated by the first such call and counted in smst_batch_workspace_bytes; a steady-state call allocates nothing and
 * adds no host synchronisation.
 * Out of scope: the planar calls (the streaming frame calls have a setting of their own: "Stream output resample" below);
 * irrational or time-varying ratios; a quality setting.
 * SMST_ERR_INVALID with a message that names the limit: the limits of "Resample", the ninth distinct ratio across the four settings
 * included; a stream index out of range; a null batch; in a call, an E that does not fit an int. */
/* stream = -1: every stream.  1/1 turns the stage off.  The first call with a ratio the batch does not have builds that ratio's table and
 * puts it into device memory: tables are never uploaded in a call */
int smst_batch_set_pcm_out_resample(smst_batch *b, int stream, int up, int down);
/* the stream's reduced output ratio (1/1: none); either pointer may be null */
int smst_batch_pcm_out_resample(const smst_batch *b, int stream, int *up, int *down);
/* E of outSamples delivered frames of the stream (outSamples itself at 1/1), or a negative code */
long long smst_batch_pcm_out_render_length(const smst_batch *b, int stream, long long outSamples);
/* test hook: the output-resample kernel alone, planar fp32 to planar fp32, as smst_debug_clip_resample (host pointers, staged whole as far
 * behind a 16-byte boundary as the caller's; a stream at 1/1 is left alone, and so is everything in `out` outside the destination runs).
 * counts: [streams] Nd; ratios: [streams][2] up, down; srcSegments: [streams][2][4] as smst_debug_clip_copy's, where the E rendered frames
 * lie in `image` (src and count: segment 0 holds the frames [0, k) at its column, segment 1 the frames [k, E) at its own; the counts add up
 * to E); dstSegments: [streams][2][4], the DESTINATION of the Nd delivered frames (dst and count; the counts add up to Nd) */
int smst_debug_clip_resample_out(int device, int streams, int channels, const int *counts, const int *ratios,
                                 const float *image, long long imageStreamStride, long long imageChannelStride, const int *srcSegments,
                                 const int *dstSegments, float *out, long long outStreamStride, long long outChannelStride);
/* ---- Stream resample (EXTENSION; opt-in: a batch that never calls smst_batch_set_pcm_stream_resample launches the kernels, writes the bytes and counts the launches it did before) ----
 * The converter above knows a whole clip.  A live 44.1 kHz source in a 48 kHz batch had to be resampled on the CPU before every
 * smst_batch_process_pcm.  The converter is a non-recursive FIR, so it has an exact streaming form: with the last T - 1 input frames carried
 * per stream and the output H input frames late, a stream cut into calls in any way hands the engine, bit for bit, the frames that the clip
 * converter makes of the same material.
 *
 * It is a per-stream setting of its own, a reduced ratio L/M with the shape H, T = 2H and the limits, table and arithmetic of "Resample", NOT
 * the whole-clip ratio: that one stays refused in the streaming calls.  A stream may carry both; each call family reads its own.
 *
 * Definition.  Let x(0), x(1), ... be the frames handed for the stream through smst_batch_process_pcm / smst_batch_seek_pcm since its line
 * was last cleared, fed their number, and R(q) = ceil(max(q, 0)*L/M) in 64-bit integers.  After fed frames the engine has been handed, in
 * order, the first made = R(fed - H) frames of "Resample" applied to the clip [x(0) ... x(fed - 1)]: frame n sits at i = (n*M)/L,
 * p = (n*M) mod L and is float32(sum_j double(c[p][j])*double(x(i + j - (H - 1)))), j ascending from 0.0, x of a negative index = +0.0.
 * Frame n is produced once i + H <= fed - 1, so the clip's right edge never enters and the result does not depend on the cuts.
 *   Frames per call.  A call that hands n frames gives the engine k = R(fed + n - H) - R(fed - H) frames; k may be 0.  The call then
 *   behaves exactly as if the caller had handed those k planar frames to smst_batch_process / _seek: the engine's rate is k/outSamples, the
 *   silence gate and everything behind it see the k frames.  k moves by +-1 from call to call where n*L/M is no integer, and the first
 *   calls are short by the latency; a caller who wants a fixed k asks smst_batch_pcm_stream_resample_need for the n that gives it.
 *   Known answers.  160/147, calls of 441 frames: k = 446, 480, 480, 480.  147/160 (H = 35), calls of 128: k = 86, 118, 117, 118.  3/2,
 *   37 frames with x(2) = 1, cut 3, 2, 32: k = 0, 0, 8, and the 8 frames are "Resample"'s known answer bca067e3 be4717b5 3ed8327b 3f7ae0ea
 *   3ed8327b be4717b5 bca067e3 3dddb185.
 *   Latency.  H frames at the stream's own rate: 32 for an upsampling ratio, ceil(32*M/L) otherwise (smst_batch_pcm_stream_resample_latency).
 *   Ending a stream.  The caller hands H frames of zeros: the engine has then been handed exactly the Nr = ceil(N*L/M) frames of the clip form.
 *   The line holds the last T - 1 planar fp32 frames of every channel; fed and made are 64-bit host counters.  No device readback and no host
 *   synchronisation is added.  It is cleared (frames <- +0.0, fed = made = 0) by the setter for the stream, by smst_batch_reset, and by
 *   smst_batch_seek_pcm for the streams that take part, BEFORE their frames go in: a seek is a jump in the source.  A stream with no frame
 *   in a call keeps its line.
 *   Mixing.  A stream without the setting gets, in the same call, the bytes it gets in a batch without any.
 *   Ratio tables.  The setting shares the batch's ratio tables and its SMST_RESAMPLE_MAX_RATIOS slots with the whole-clip setting: a slot is
 *   live while any of the four resample settings of any stream uses it.
 *
 * How.  In a call where a stream of the batch has the setting, the frame conversion runs once per destination that has frames -- the plain
 * streams into the engine's input image as ever, the others into a raw planar image -- and one kernel (csrc/smst_stream_resample.h;
 * DESIGN.md) forms the k frames of each such stream into the engine's image, staging every tile's input span from the line and the raw
 * image, by the clip converter's own tap sum (one device function for both); the workgroup behind a stream's last tile writes its new
 * line.  The lines exist twice, a call reads one set and writes the other, and everything is ordered by the batch's stream.  Lines and call
 * tables live in device memory, allocated by the first setter call with a ratio other than 1/1, never in a call, and counted in
 * smst_batch_workspace_bytes; the raw image grows with the first call that needs it; a steady-state call allocates nothing.
 * Out of scope: the planar calls (resampling the output in the streaming calls: "Stream output resample" below); smst_batch_output_seek_pcm; stretch_cli (a whole-file tool, which has --rate);
 * time-varying ratios.
 * SMST_ERR_INVALID with a message, before anything runs: the limits of "Resample"; a stream index out of range; a null batch;
 * smst_batch_output_seek_pcm and smst_batch_exact_pcm with a participating stream that has the setting (smst_batch_exact_pcm has
 * smst_batch_set_pcm_resample); a k or a count that does not fit an int. */
/* stream = -1: every stream.  1/1 turns the setting off.  Clears the line of the stream(s).  The first call with another ratio allocates the
 * lines and the call tables, and builds the ratio's table where the batch does not have it yet */
int smst_batch_set_pcm_stream_resample(smst_batch *b, int stream, int up, int down);
/* the stream's reduced ratio (1/1: none); either pointer may be null */
int smst_batch_pcm_stream_resample(const smst_batch *b, int stream, int *up, int *down);
/* H of the stream's ratio, the frames at the stream's own rate by which its input is late; 0 without the setting */
int smst_batch_pcm_stream_resample_latency(const smst_batch *b, int stream, int *frames);
/* k of the stream's next call if it hands inSamples frames (inSamples itself without the setting), or a negative code.  fresh != 0: as after
 * a clear -- what the call behind a seek or a reset gives */
long long smst_batch_pcm_stream_resample_frames(const smst_batch *b, int stream, long long inSamples, int fresh);
/* the smallest n whose call gives the engine k >= frames, frames >= 1: max(0, ((made + frames - 1)*M)/L + H + 1 - fed) (frames itself
 * without the setting), or a negative code */
long long smst_batch_pcm_stream_resample_need(const smst_batch *b, int stream, long long frames, int fresh);
/* test hook: `calls` launches of the stream-resample kernel in sequence, with the carried lines, planar fp32 to planar fp32 (host pointers,
 * strides in floats, staged whole as far behind a 16-byte boundary as the caller's).  counts: [calls][streams], negative = the stream takes
 * no part in that call; ratios: [streams][2] up, down (1/1: the stream's rows of `out` are left alone); fed0: [streams] or null -- the line
 * starts as zeros at that position (fed = fed0, made = R(fed0 - H)); image: each stream's frames in order from column 0 of its rows; out:
 * each stream's frames as made, in order from column 0, at most maxFrames of them; made: [streams], the frames written (may be null) */
int smst_debug_pcm_stream_resample(int device, int streams, int channels, int calls, const int *counts, const int *ratios, const long long *fed0,
                                   const float *image, long long imageStreamStride, long long imageChannelStride,
                                   float *out, long long outStreamStride, long long outChannelStride, int maxFrames, long long *made);
/* ---- Stream output resample (EXTENSION; opt-in: a batch that never calls smst_batch_set_pcm_stream_out_resample launches the kernels, writes the bytes and counts the launches it did before) ----
 * "Output resample" delivers whole clips at their own rate; "Stream resample" takes a live stream at its own rate.  A live stream could not
 * be DELIVERED at its own rate: a 44.1 kHz device fed from a 48 kHz batch copied every quantum back and resampled it on the CPU, behind the
 * stream limiter, the stream meter, the gain, the dither and the overs counter, which then described frames that were not the ones
 * delivered.  The converter is a non-recursive FIR, so it has an exact streaming form behind the engine as it has in front of it.
 *
 * It is a per-stream setting of its own beside the whole-clip output ratio (smst_batch_set_pcm_out_resample), which stays refused in the
 * streaming calls.  The ratio L/M = up/down is the DELIVERY rate over the batch's rate, reduced by the library, with the limits, the table,
 * the shape (H, T = 2H) and the arithmetic of "Resample"; it is one more user of the batch's SMST_RESAMPLE_MAX_RATIOS shared table slots: a
 * slot is live while any of the four settings of any stream uses it.  The setting makes smst_batch_process_pcm and smst_batch_flush_pcm
 * deliver the stream's frames at the delivery rate.
 *
 * Definition.  Let r(0), r(1), ... be the frames the engine has emitted for the stream through smst_batch_process_pcm / _flush_pcm since its
 * line was last cleared, and `delivered` the number of frames the caller has received since then, a 64-bit host counter.  All integers
 * below are 64-bit.
 *   Lengths.  outSamples[s] stays what the caller receives: Nd frames at the delivery rate.  The engine renders
 *   E = ceil((delivered + Nd)*M/L) - ceil(delivered*M/L) frames; E may be 0 and must fit an int.  E depends on nothing but `delivered` and
 *   Nd: it has no burst and no term in H.  Towards the engine the call behaves exactly as if the caller had asked for E frames: the
 *   engine's rate is fed/E, and a call with E = 0 is what smst_batch_process with a zero output count is.  In a flush the engine's flush
 *   gets E; its `rates` stay relative to frames at the batch's rate.  Nothing in the call's interface is sized by E
 *   (smst_batch_pcm_stream_out_resample_render reports it).
 *   Latency.  Dl = ceil(H*L/M) delivered frames (smst_batch_pcm_stream_out_resample_latency): 64 at 2/1, 32 at 1/2, 48 at 3/2, 32 at 2/3,
 *   35 at 160/147, 33 at 147/160, 33 at 147/640, 140 at 640/147.  Delivered frame n < Dl is +0.0.  Delivered frame n >= Dl is frame
 *   m = n - Dl of "Resample" applied to r: i = (m*M)/L, p = (m*M) mod L, and the value is
 *   float32(sum_j double(c[p][j])*double(r(i + j - (H - 1)))), j ascending from 0.0, r of a negative index = +0.0.  Because Dl*M/L >= H,
 *   every such frame has i + H <= ceil((n + 1)*M/L) - 1: the right edge of what has been rendered never enters, and the result does not
 *   depend on how the stream is cut into calls (csrc/smst_stream_resample_out.h has the proof).
 *   Known answers.  147/160, calls of 128 delivered frames: E = 140, 139, 139, 140.  160/147, calls of 480: E = 441 every call.  3/2,
 *   calls of 16: E = 11, 11, 10.  3/2, mono, r(2) = 1 and 0 elsewhere, calls of 20, 28, 8: E = 14, 18, 6; the delivered frames 0 ... 47 are
 *   +0.0 and the frames 48 ... 55 are "Resample"'s known answer bca067e3 be4717b5 3ed8327b 3f7ae0ea 3ed8327b be4717b5 bca067e3 3dddb185.
 *   2/3, r(3) = 1: the delivered frames 32 ... 36 are bc55dff0 3c594cd8 3f2740ad 3c594cd8 bc55dff0.
 *   Ending a stream.  The caller asks its flush for Dl frames more: the engine's flush emits zeros beyond its tail, so the last frames are
 *   the clip form's.
 *   The line.  Per stream and channel, the last rendered frames that a later call can still reach.  The next call's first frame reaches
 *   back to ((delivered - Dl)*M)/L - (H - 1), at most T + ceil(M/L) frames below ceil(delivered*M/L): 293 at 2/9.  It is cleared
 *   (frames <- +0.0, delivered = 0) by the setter for the stream and by smst_batch_reset.  It is NOT cleared by smst_batch_seek_pcm or
 *   smst_batch_output_seek_pcm -- they emit nothing, and the output timeline goes on -- nor by a flush.  A stream with no frame in a call
 *   keeps its line.
 *   Everything behind the converter runs on the delivered frames: the stream limiter (whose latency adds to Dl), the stream meter (its
 *   v(n) are the delivered frames, the Dl zeros included; the caller gives it the DELIVERY rate), gain, dither (whose frame index is the
 *   delivered frame's), conversion, overs and peaks.
 *   The setting may be combined with smst_batch_set_pcm_stream_resample on the same stream: 44.1 kHz in, a 48 kHz batch, 44.1 kHz out.
 *   Mixing.  A stream without the setting gets, in the same call, the bytes it gets in a batch without any.
 *
 * How.  The engine renders every stream's frames into its output image as ever -- E of them for a stream with the setting; the image's rows
 * hold max(E, Nd) frames.  One kernel (csrc/smst_stream_resample_out.h) forms the Nd delivered frames of each such stream into
 * a second image, staging every tile's span from the stream's line and the frames just rendered, by the clip converter's own tap sum (one
 * device function for all four converters); the workgroup behind a stream's last tile writes its new line.  A small second kernel copies
 * the delivered frames back over those streams' rows of the engine's image, and the stream limiter, the stream meter and the conversion
 * read that one image as they did; plain streams are never touched.  The lines exist twice, a call reads one set and writes the other, and
 * everything is ordered by the batch's stream.  Lines and call tables live in device memory, allocated by the first setter call with a ratio
 * other than 1/1, never in a call, and counted in smst_batch_workspace_bytes; the second image grows with the first call that needs it; a
 * steady-state call allocates nothing, and no host synchronisation and no device readback is added.
 * Out of scope: the planar calls (they neither serve nor refuse the setting, as with "Stream resample"); stretch_cli (a whole-file tool,
 * which has --out-rate); time-varying or irrational ratios; a quality setting.
 * SMST_ERR_INVALID with a message, before anything runs: the limits of "Resample", the ninth distinct ratio across all four settings
 * included; a stream index out of range; a null batch; an E that does not fit an int; smst_batch_exact_pcm with a participating stream that
 * has the setting (it has smst_batch_set_pcm_out_resample). */
/* stream = -1: every stream.  1/1 turns the setting off.  Clears the line of the stream(s).  The first call with another ratio allocates the
 * lines and the call tables, and builds the ratio's table where the batch does not have it yet */
int smst_batch_set_pcm_stream_out_resample(smst_batch *b, int stream, int up, int down);
/* the stream's reduced ratio (1/1: none); either pointer may be null */
int smst_batch_pcm_stream_out_resample(const smst_batch *b, int stream, int *up, int *down);
/* Dl of the stream's ratio, the delivered frames by which its output is late; 0 without the setting */
int smst_batch_pcm_stream_out_resample_latency(const smst_batch *b, int stream, int *frames);
/* E of the stream's next call if it delivers outSamples frames (outSamples itself without the setting), or a negative code.  fresh != 0: as
 * after a clear -- what the call behind a reset gives */
long long smst_batch_pcm_stream_out_resample_render(const smst_batch *b, int stream, long long outSamples, int fresh);
/* test hook: `calls` launches of the stream-output-resample kernel in sequence, with the carried lines, planar fp32 to planar fp32 (host
 * pointers, strides in floats, staged whole as far behind a 16-byte boundary as the caller's).  counts: [calls][streams] Nd, negative = the
 * stream takes no part in that call; ratios: [streams][2] up, down (1/1: the stream's rows of `out` are left alone); delivered0: [streams]
 * or null -- the line starts as zeros at that position (delivered = delivered0); image: each stream's rendered frames in order from column
 * 0 of its rows; out: each stream's delivered frames, in order from column 0, at most maxFrames of them; rendered: [streams], the frames
 * of `image` consumed (may be null) */
int smst_debug_pcm_stream_resample_out(int device, int streams, int channels, int calls, const int *counts, const int *ratios, const long long *delivered0,
                                       const float *image, long long imageStreamStride, long long imageChannelStride,
                                       float *out, long long outStreamStride, long long outChannelStride, int maxFrames, long long *rendered);
/* ---- Stream meter (EXTENSION; opt-in: a batch that never calls smst_batch_set_pcm_stream_meter launches the kernels, writes the bytes and counts the launches it did before) ----
 * The meters above ("Loudness", "True peak", "Loudness range") know a whole clip.  A live bus could be stretched, resampled, levelled and
 * limited on the device, but to learn its loudness the caller had to copy the output back and meter it on the host.  Each meter has an exact
 * streaming form: a small carried state per stream, and a definition that makes the readings equal to the clip meters' bit for bit, however
 * the stream is cut into calls.
 *
 * It is a per-stream setting of its own beside the whole-clip flags, which stay refused in the streaming calls.  With it on, every frame that
 * smst_batch_process_pcm and smst_batch_flush_pcm write for the stream is measured on the device, behind the call's last emitting kernel:
 * no host synchronisation in the call, no allocation in the call, no floating-point atomic.  The caller asks for the readings at any time.
 *
 * Definition.  Let v(n), n = 0 ... T - 1, be the frames the engine has emitted for the stream through smst_batch_process_pcm /
 * smst_batch_flush_pcm since the meter was last cleared -- BEFORE the gain, as every other meter of the library measures, and at emission, not
 * where a stream limiter delays them.  Let h = round(fs/10) and Tm = min(T, maxSubBlocks*h).  After any call the readings are, bit for bit,
 * what smst_debug_clip_loudness_range (the four loudness passes and the range stage) and smst_debug_clip_true_peak report of the clip
 * v[0, Tm) with the same fs and the batch's channel weights.  Nothing else defines the result: not how T was cut into calls, not which
 * update form ran.
 *   K-weighting.  The clip meter enters chunk k + 1 of SMST_LOUDNESS_CHUNK = 256 frames with A^256 x_in[k] + ends[k], ends[k] the state chunk
 *   k reaches from ZERO state.  The stream meter keeps that chunk grid, anchored at n = 0, and carries per (stream, channel), all float64,
 *   for the chunk in progress: x_in, the state run from x_in, the state run from zero, and the two partial sums e0, e1.
 *   Sub-block sums.  The clip meter adds a sub-block's partials from 0.0 in chunk order, so the running sum of the sub-block in progress is
 *   carried too.  Sub-block j closes when position (j + 1)*h is reached, which may fall inside a chunk whose e0 is by then complete.
 *   One source form.  The filter step, the accumulation e += y*y and the chunk carry are one source expression each, shared with the clip
 *   passes (the library is built with -ffp-contract=on: the source form decides the fusing).
 *   History.  The relative gates and the percentiles need every block of the programme: per metered stream the device keeps the closed
 *   sub-block sums sub[c][j], j < maxSubBlocks, appended by the update and never rewritten.  A reading runs the clip meter's own stages on
 *   them -- sub-block sums -> block powers -> the two gates, then the range stage --, so everything behind the sums is identical by construction.
 *   True peak.  The clip definition has zeros beyond the clip's end, so the windows of n >= T - 6 change when more frames arrive.  The
 *   update folds only COMPLETE windows (n <= Tm - 7) into the running word, every sample |x(n)| at once, and carries the last 11 frames of
 *   every channel.  A reading computes the six edge windows against zeros from the carried frames and reports max(running, edge) without
 *   folding the edge in: a later reading may be LOWER.  The running word starts at 0, the carried frames at +0.0 (the clip's "x outside
 *   [0, N) is 0").
 *   Capacity.  maxSubBlocks is given with the setting and sizes the history: 100-ms sub-blocks, `channels` doubles each.  A full meter
 *   freezes -- it refuses no call --, true peak at the same frame, so one Tm describes all readings.  The batch's histories are allocated by
 *   the first setter call with on != 0, for its maxSubBlocks; a later call may ask for at most that many.
 *   NaN and inf behave as in the clip meters: a NaN poisons the filter from there on and is skipped by the peak.
 *   Which calls.  smst_batch_process_pcm and smst_batch_flush_pcm meter the frames they write for a stream with the setting.  A stream with no
 *   frame in a call, or left out of a flush, keeps its state.  The seek calls emit nothing and meter nothing.
 *   Clearing.  By the setter (for that stream) and by smst_batch_reset; not by a level, limiter or weights change.
 *   smst_batch_set_pcm_loudness_weights while a meter holds frames is refused: the clip equivalence has one weight set.
 *   Mixing.  The meter changes NO output byte of any stream; an unflagged stream's bytes and meters are what they are without it.
 *   A reading describes v before the gain: a FIXED gain g adds 20*log10|g| LU to every loudness.
 *
 * How.  Behind the output conversion of a call in which a metered stream has frames, kPcmStreamMeterPeak (one lane per new frame: the sample
 * and the window that the frame completes, integer maxima) and the update run on the batch's stream (csrc/smst_stream_meter.h).
 * The update has two forms, which give the same bits; the host chooses by the call's longest metered count (SMST_STREAM_METER_SCAN_FRAMES).
 * The short-call form, kPcmStreamMeter: one lane per (stream, channel), its row staged through LDS in tiles, continues the chunk in progress
 * and appends the sub-block sums that close.  The chunk-scan form: the clip meter's three passes with a start position and the carried state
 * -- a zero-state pass over the call's chunks whose first chunk resumes the carried zero-state run, the carry chain from the carried x_in,
 * an energy pass whose last chunk, if incomplete, leaves the carried state -- and a pass that closes the sub-block sums in chunk order; its
 * scratch grows with the first call that needs it, as the images do.  One set of carried state serves calls in flight: a lane updates the
 * state of its own (stream, channel) only, the kernels in front of it only read what is carried, and everything is ordered by the batch's
 * stream.  A take runs the gate stage, the range stage and one small kernel for the true-peak edge on the histories.
 * The equality covers the sign of a NaN: where both operands of a product or a sum can be NaN -- the chunk carry and the sub-block sums at a
 * rate below 3364 Hz, where the K-weighting shelf is unstable and A^256 is not finite -- the operand order is written down, one device
 * function for the clip passes and both update forms.
 * Out of scope: metering the signal behind the gain or the stream limiter; the planar calls; stretch_cli (a whole-file tool, which has the
 * clip meters); a sliding "last N minutes" integrated window; a per-stream weight set; a histogram-gated approximate meter with unbounded
 * programme length.
 * SMST_ERR_INVALID with a message: a null batch; a stream index out of range; with on != 0 a rate that smst_batch_set_pcm_loudness would
 * refuse, maxSubBlocks < 1, maxSubBlocks*h >= 2^31 or maxSubBlocks above what the histories were allocated for; smst_batch_exact_pcm with a
 * participating stream that has the setting (the whole-clip flags are the clip form). */
/* stream = -1: every stream.  Clears the stream's meter (T = 0), on or off.  sampleRate by the rule of smst_batch_set_pcm_loudness
 * (h >= SMST_LOUDNESS_CHUNK); maxSubBlocks >= 1, read with on != 0 only.  The first call with on != 0 allocates the carried state and the
 * histories (counted in smst_batch_workspace_bytes) -- never a streaming call */
int smst_batch_set_pcm_stream_meter(smst_batch *b, int stream, int on, double sampleRate, int maxSubBlocks);
int smst_batch_pcm_stream_meter(const smst_batch *b, int stream, int *on, double *sampleRate, int *maxSubBlocks);
/* host counters, no synchronisation: frames emitted for the stream since the clear (T) and frames metered (Tm) */
int smst_batch_pcm_stream_meter_frames(const smst_batch *b, int stream, long long *frames, long long *metered);
/* per stream, of v[0, Tm): integrated loudness and its two block counts; the NEWEST momentary and short-term loudness (z of block nb - 1,
 * st of block ns - 1; -inf where there is none); their maxima; LRA, low, high, ns, n; the true peak and the sample peak.  Values and
 * conventions as smst_batch_take_pcm_loudness / _loudness_range / _true_peaks report them.  Any pointer may be null.  Synchronises the
 * batch; resets nothing: metering goes on */
int smst_batch_take_pcm_stream_meter(smst_batch *b, double *lufs, int *blocks, int *gated, double *momentary, double *shortTerm,
                                     double *momentaryMax, double *shortTermMax, double *range, double *low, double *high,
                                     int *shortBlocks, int *rangeBlocks, float *truePeaks, float *samplePeaks);
/* test hook: `calls` meter updates in sequence on one device stream over a planar fp32 image that holds each stream's frames in order
 * (counts: [calls][streams], negative = takes no part), a reading after every call k with readAfter[k] != 0 (null: after the last only).
 * Readings are POWERS, as smst_debug_clip_loudness_range reports them, reading-major: Z[r*streams + s] ...; blockPowers / shortPowers of the
 * LAST reading only ([streams][maxBlocks]).  flags: [streams], 0 = the stream is not metered (null: every one is).  form: 0 = the library's
 * own choice per call, 1 = force the short-call form, 2 = force the chunk-scan form */
int smst_debug_pcm_stream_meter(int device, int streams, int channels, int calls, const int *counts, const int *readAfter, int form,
                                const float *image, long long imageStreamStride, long long imageChannelStride,
                                const double *sampleRates, const float *weights, const int *flags, int maxSubBlocks,
                                double *Z, int *blocks, int *gated, double *momentaryMax, double *shortTermMax, double *low, double *high,
                                int *shortBlocks, int *rangeBlocks, float *truePeaks, float *samplePeaks, long long *metered,
                                double *blockPowers, double *shortPowers, int maxBlocks);
/* per stream, since the last take: peaks[s] = the largest |v| the levelled output conversions met BEFORE the gain (0 if none); gains[s] = the
 * gain the newest levelled conversion of stream s applied (1 before any).  Either may be null.  Synchronises the batch; resets the peaks,
 * not the gains. */
int smst_batch_take_pcm_peaks(smst_batch *b, float *peaks, float *gains);
/* test hook: smst_debug_pcm_convert_dithered through the levelled kernel, with per-stream fixed gains ([streams]); peaks ([streams], may be
 * null): the peaks it metered */
int smst_debug_pcm_convert_levelled(int device, int format, int streams, int channels, const int *counts,
                                    const void *src, long long srcStreamStride, long long srcInnerStride,
                                    void *dst, long long dstStreamStride, long long dstInnerStride,
                                    const int *modes, const long long *seeds, const long long *firstFrames, const float *gains,
                                    long long *clamped, long long *nans, float *peaks);
/* test hook: smst_debug_clip_copy for dir 1 into a frame format through the peak pass and the levelled copy kernel, with per-stream level
 * entries (levelModes, gains, ceilings) and dither entries (ditherModes, seeds; the frame index is the place in the clip) ([streams] each);
 * peaks / applied ([streams], either may be null): the peaks it metered and the gains it applied (1 for a stream that moved no sample) */
int smst_debug_clip_copy_levelled(int device, int format, int streams, int channels, const int *segments,
                                  const void *src, long long srcStreamStride, long long srcInnerStride,
                                  void *dst, long long dstStreamStride, long long dstInnerStride,
                                  const int *levelModes, const float *gains, const float *ceilings, const int *ditherModes, const long long *seeds,
                                  long long *clamped, long long *nans, float *peaks, float *applied);
/* test hook: the two conversion kernels alone, ragged counts, arbitrary strides; dir 0 = PCM -> planar, 1 = planar -> PCM.  Host pointers: the
 * PCM side is (stream stride, frame stride), the planar side (stream stride, channel stride), in elements.  Both buffers are staged whole (what
 * the kernel leaves alone in `dst` comes back as it was) into device buffers offset from a 16-byte boundary as the caller's pointers are.
 * Synchronises before it returns. */
int smst_debug_pcm_convert(int device, int dir, int format, int streams, int channels, const int *counts,
                           const void *src, long long srcStreamStride, long long srcInnerStride,
                           void *dst, long long dstStreamStride, long long dstInnerStride);
/* Overs.  The output conversions of process_pcm and flush_pcm count, per stream, the elements they could not represent: clamped[s] = those
 * whose code the clamp set (integer formats) or that became +-inf from a finite value (float16); nans[s] = those whose input was NaN (every
 * format, float32 included).  The counters ([streams][2], 32 bits each, device memory allocated with the batch and part of
 * smst_batch_workspace_bytes) are added to by the conversion kernel itself: the calls allocate and synchronise nothing for them. */
/* overs of the _pcm output conversions (process_pcm, flush_pcm) since the last take, per stream; either pointer may be null.
 * Synchronises the batch. */
int smst_batch_take_pcm_overs(smst_batch *b, long long *clamped, long long *nans);
/* smst_debug_pcm_convert for dir 1, also returning the counts the kernel made ([streams] each) */
int smst_debug_pcm_convert_counted(int device, int format, int streams, int channels, const int *counts,
                                   const void *src, long long srcStreamStride, long long srcInnerStride,
                                   void *dst, long long dstStreamStride, long long dstInnerStride,
                                   long long *clamped, long long *nans);
/* test hook: the planar -> PCM kernel alone with per-stream dither ([streams] each: modes, seeds, the frame index of each stream's first
 * frame), staged as smst_debug_pcm_convert_counted stages its buffers; clamped / nans: either may be null.  A launch in which a stream has a
 * mode is the dithered kernel (int16 / int24; the other formats have none). */
int smst_debug_pcm_convert_dithered(int device, int format, int streams, int channels, const int *counts,
                                    const void *src, long long srcStreamStride, long long srcInnerStride,
                                    void *dst, long long dstStreamStride, long long dstInnerStride,
                                    const int *modes, const long long *seeds, const long long *firstFrames,
                                    long long *clamped, long long *nans);
/* test hook: the two copy kernels of the exact calls alone (csrc/smst_clip.h).  dir 0 = caller's buffer -> planar image, 1 = planar image ->
 * caller's buffer; format: an SMST_PCM_* code (the caller's side is frames: stream stride, frame stride) or 0 (it is planar fp32 itself: stream
 * stride, channel stride); the image side is always (stream stride, channel stride); strides in elements.  segments: [streams][2][4] host ints
 * (source frame, destination frame, count, zeros): `count` frames from frame `source` of the stream's row(s) in src to frame `destination` in
 * dst; zeros != 0 (dir 1): no source, the destination gets 0.0.  Host pointers; both buffers are staged whole -- as far as the segments reach --
 * (what the kernel leaves alone in `dst` comes back as it was) into device buffers offset from a 16-byte boundary as the caller's pointers are.
 * clamped / nans (either may be null): [streams], the overs the kernel counted (dir 1 into a frame format).  Synchronises before it returns. */
int smst_debug_clip_copy(int device, int dir, int format, int streams, int channels, const int *segments,
                         const void *src, long long srcStreamStride, long long srcInnerStride,
                         void *dst, long long dstStreamStride, long long dstInnerStride,
                         long long *clamped, long long *nans);
int smst_batch_synchronize(smst_batch *b);
/* raw hipStream_t the batch enqueues on (so callers can order their own device work against it) */
void *smst_batch_hip_stream(smst_batch *b);
/* Stream ordering for device-memory callers, without a host synchronisation:
 * wait_for_stream: everything the batch enqueues from now on runs after the work ALREADY enqueued on `hipStream` (the
 *                  caller's producer of the input tensors); call it before smst_batch_process / _seek / _output_seek.
 * signal_stream:   work enqueued on `hipStream` from now on runs after everything the batch has enqueued so far (so a
 *                  consumer of the outputs need not call smst_batch_synchronize). */
int smst_batch_wait_for_stream(smst_batch *b, void *hipStream);
int smst_batch_signal_stream(smst_batch *b, void *hipStream);

/* measurement hooks: per-kernel-class device time (hipEvent pairs on the batch's stream) accumulated since the
 * last call.  ms[0..6] = analyse, feed, predict, chain, synth, emit, other; launches[0..4] = analyse, predict,
 * chain, synth, emit. */
/* mode 1: HIP-event pairs around every kernel class, tiles serialised (ms[0..6]: analyse, feed, predict, recurrence, synth,
 * emit, other; launches[0..4]: analyse, predict, recurrence, synth, emit).  mode 2: only the recurrence kernel, timed in
 * place on its own stream while the other streams keep overlapping it (ms[7], launches[5]).  0: off. */
int smst_batch_enable_profiling(smst_batch *b, int mode);
int smst_batch_take_timings(smst_batch *b, double ms[8], long long launches[6]);
/* Host time of smst_batch_process since the last take (always counted, no mode): ms[0] wall time inside the calls, of which ms[1] was spent
 * waiting for the call before the previous one to finish (two sets of per-call tables: the host runs at most two calls ahead of the device --
 * back-pressure, not work) and ms[2] waiting for the silence gate's readback; ms[0] - ms[1] - ms[2] is the host's own work (block scheduler,
 * table fills, enqueues).  *calls (may be null): the number of calls.  One host thread per batch: its work must stay below the device's step. */
int smst_batch_take_host_times(smst_batch *b, double ms[3], long long *calls);

/* test hooks (tests/ only): per-stream state rows.  which: 0 Band.input, 1 Band.prevInput, 2 Band.output
 * (interleaved re,im: 2*channels*bands floats), 3 Prediction.energy (channels*bands floats). */
int smst_batch_debug_get_state(smst_batch *b, int stream, int which, float *dst);
int smst_batch_debug_get_carry(smst_batch *b, int stream, float *sums, float *products);
/* teacher forcing (SURVEY.md App. D.2 i): overwrite one stream's carried per-bin state (same selectors / layouts as
 * the getters) or its overlap-add carry ([channels][block+interval] sums, [block+interval] window products, index 0 =
 * the next output sample).  The batch is synchronised first. */
int smst_batch_debug_set_state(smst_batch *b, int stream, int which, const float *src);
int smst_batch_debug_set_carry(smst_batch *b, int stream, const float *sums, const float *products);
/* number of device / pinned allocations and host-table growth events since the batch was created.  process() is
 * allocation-free in steady state (the reference asserts the same of itself: cmd/main-dev.cpp:158-163, "allocated during
 * process()"): tests/test_abi.py::test_process_does_not_allocate_in_steady_state checks that this number stands still. */
long long smst_batch_debug_allocation_events(const smst_batch *b);
/* output map of the stream's newest hop (2*bands floats: inputBin, freqGrad per bin; signalsmith-stretch.h:587-590,
 * :882-917).  Returns 1 if that hop had a frequency map, 0 if not (dst untouched), negative on error. */
int smst_batch_debug_get_map(smst_batch *b, int stream, float *dst);
/* the formant stage of the stream's newest hop (signalsmith-stretch.h:972-1036): ratio[bands] = the per-bin energy ratio applied to every channel's
 * inputEnergy (:1026-1033), envelope[bands] = formantMetric after its eight max-decay / min-grow passes (:984-1006), *freqEstimate = the pitch
 * estimate in bins the envelope was built with (:980-981, :929-966).  Available only in a batch created with SMST_NO_FEED_FUSION=1 (the separate
 * envelope kernel writes them; the default form keeps them in LDS and is bit-identical to it: test_feed_fusion_equals_separate).  Returns 1, or 0
 * if that hop had no formant processing / the batch runs the fused kernels (destinations untouched), negative on error. */
int smst_batch_debug_get_formants(smst_batch *b, int stream, float *ratio, float *envelope, float *freqEstimate);
/* the kernels' packed complex helpers (csrc/smst_complex.h, gfx950 inline assembly) evaluated on the device: in = n x
 * (a.re, a.im, b.re, b.im, c.re, c.im, fraction), out = n x (a*b, a*conj(b), a*b + c, a + (b - a)*fraction) as 8 floats. */
int smst_debug_complex_selftest(int device, const float *in, float *out, int n);
/* the FFT kernels' complex helpers (csrc/smst_fft_complex.h) likewise: in = n x (a.re, a.im, b.re, b.im), out = n x (a*b, a*conj(b) as the
 * inverse transform's twiddle product rounds it, a*conj(b) as the windowed store rounds it, a + i*b, a - i*b, a + b, a - b, conj(a) from the
 * conjugating store, conj(a) from the conjugating load, a through both with the condition false) as 20 floats. */
int smst_debug_fft_complex_selftest(int device, const float *in, float *out, int n);
/* launches, since the library was loaded, of one kernel variant: "vocoder_aligned", "vocoder_staged", "vocoder_gather",
 * "vocoder_n", "vocoder_one", "vocoder_across", "vocoder_continuous", "chain_unfused", "analyse_teams", "analyse_pairs" (the two-frames-per-pass form of the analysis teams: such a launch counts in both), "analyse_fast", "analyse_generic",
 * "synth_teams", "synth_fast", "synth_generic", "synth_emit", "emit_carried", "feed_one_pass", "pcm_in", "pcm_out" (the conversion kernels of the _pcm calls, whatever
 * the format), "clip_in", "clip_out" (the copy kernels of the exact calls, planar or any format), "pcm_out_dithered", "clip_out_dithered" (a launch in
 * which at least one stream dithers into int16 or int24 counts here INSTEAD of "pcm_out" / "clip_out") (-1: unknown name).  The "this form is bit-identical to that form" tests
 * assert through it that both forms really ran. */
long long smst_debug_launch_count(const char *name);

#ifdef __cplusplus
}
#endif
#endif /* SMST_H */
