/*
 * dsmi.h -- C ABI of libdsmi.so: the MI355X-native (gfx950) implementation of the
 * DanSpeech recognize() hot path.
 *
 * The reference (danspeech/danspeech, pure Python) has no FFI of its own; its only
 * boundary for this path is the Python call chain
 *     Recognizer.recognize            danspeech/Recognizer.py:82-95
 *       -> DanSpeechRecognizer.transcribe   danspeech/DanSpeechRecognizer.py:218-231
 *            -> SpectrogramAudioParser.parse_audio  danspeech/audio/parsers.py:50-72
 *            -> DeepSpeech.forward                  danspeech/deepspeech/model.py:496-515
 *            -> {Greedy,BeamCTC}Decoder.decode      danspeech/deepspeech/decoder.py:129-144,183-198
 * Each entry point below names the reference interface it replaces.  The Python
 * mirror of those classes (package danspeech_amd) binds these symbols with ctypes;
 * INTEGRATION.md shows the stub a maintainer of the reference would add.
 *
 * Conventions
 *  - every function returns 0 on success and a negative dsmi_status on failure;
 *    dsmi_last_error() gives the message of the last failure on that handle
 *    (NULL handle: last failure of a create call on this thread).
 *  - "dev" pointers are HIP device pointers on the handle's device; "host" pointers
 *    are ordinary host memory.  The caller owns every buffer passed in; the library
 *    owns weights and workspaces inside the handle.
 *  - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Work is
 *    enqueued on it; functions that return host data synchronise that stream.
 *  - one handle = one GPU; distinct handles may be used from distinct threads, one
 *    handle is not re-entrant (same contract as a reference Recognizer instance).
 */
#ifndef DSMI_H
#define DSMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* libdsmi.so is built with -fvisibility=hidden: the declarations between this push and the pop at the end of the file are its whole
 * export list (tests/test_abi.py compares `nm -D` with them). */
#if defined(DSMI_BUILD) && defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

typedef enum {
    DSMI_OK = 0,
    DSMI_ERR_INVALID = -1,     /* bad argument / shape                               */
    DSMI_ERR_CONV = -2,        /* conv_layers outside 1..3 (reference ConvError, model.py:344-348) */
    DSMI_ERR_NOT_READY = -3,   /* tensor missing / finalize not called (ModelNotInitialized) */
    DSMI_ERR_UNSORTED = -4,    /* lengths not sorted descending (torch RuntimeError from
                                  pack_padded_sequence, model.py:117)                */
    DSMI_ERR_HIP = -5,         /* HIP runtime failure                                */
    DSMI_ERR_NOMEM = -6,
    DSMI_ERR_IO = -7,          /* LM file unreadable / malformed                     */
    DSMI_ERR_CAPACITY = -8,    /* batch/time exceeds dsmi_reserve()                  */
    DSMI_ERR_TIMEOUT = -9,     /* a persistent recurrent kernel's hand-off wait timed out and the batch could not be recomputed */
    DSMI_ERR_COMM = -10,       /* RCCL unavailable or an exchange failed (dsmi_comm_*)                                           */
    DSMI_RECOMPUTED = 1        /* dsmi_forward_status: the batch was recomputed on the per-step path; results valid now */
} dsmi_status;

enum { DSMI_RNN_GRU = 0, DSMI_RNN_LSTM = 1, DSMI_RNN_TANH = 2 };
enum { DSMI_WIN_HAMMING = 0, DSMI_WIN_HANN = 1, DSMI_WIN_BLACKMAN = 2, DSMI_WIN_BARTLETT = 3 };
/* Sample formats of dsmi_features.  The last three and DSMI_PCM_STEREO are the raw frames of a PCM WAV
 * file as danspeech.audio.load_audio reads them (resources.py:22-61): little-endian, unsigned 8-bit
 * biased by 128 (resources.py:551-554), and for two channels interleaved L,R frames folded on the
 * device into the SATURATING sum L+R of audioop.tomono(buf, width, 1, 1) (resources.py:302-303).
 * OR DSMI_PCM_STEREO into I16 / I24 / I32; sample counts and offsets are then in frames. */
enum { DSMI_PCM_I16 = 0, DSMI_PCM_F32 = 1, DSMI_PCM_F64 = 2, DSMI_PCM_U8 = 3, DSMI_PCM_I24 = 4, DSMI_PCM_I32 = 5,
       DSMI_PCM_STEREO = 16 };
enum { DSMI_PAD_REFLECT = 0, DSMI_PAD_CONSTANT = 1 };

/* Mirrors the arguments of DeepSpeech.__init__ (model.py:293-294) plus audio_conf
 * (danspeech/deepspeech/utils.py:1-8). */
typedef struct {
    int32_t conv_layers;        /* 1..3                                   */
    int32_t rnn_type;           /* DSMI_RNN_*                             */
    int32_t rnn_hidden_size;
    int32_t rnn_layers;
    int32_t bidirectional;      /* 0/1                                    */
    int32_t context;            /* Lookahead context (unidirectional)     */
    int32_t n_labels;           /* len(labels)                            */
    int32_t sample_rate;        /* audio_conf["sampling_rate"]  (fixes n_freq, model.py:340-355) */
    double  window_size;        /* audio_conf["window_size"], seconds     */
} dsmi_model_desc;

/* Mirrors AudioParser.__init__ (danspeech/audio/parsers.py:18-30, 43-48): audio_conf. */
typedef struct {
    int32_t sample_rate;        /* audio_conf["sampling_rate"]            */
    double  window_size;        /* seconds; n_fft = int(rate * size), double arithmetic as in Python */
    double  window_stride;      /* seconds; hop   = int(rate * stride)    */
    int32_t window;             /* DSMI_WIN_*                             */
    int32_t normalize;          /* 0/1                                    */
    int32_t pad_mode;           /* DSMI_PAD_*: librosa's centre padding (reflect <= 0.9, constant >= 0.10) */
} dsmi_frontend_desc;

typedef struct dsmi_model dsmi_model;        /* a DeepSpeech instance on one GPU          */
typedef struct dsmi_frontend dsmi_frontend;  /* a SpectrogramAudioParser on one GPU       */
typedef struct dsmi_decoder dsmi_decoder;    /* a GreedyDecoder / BeamCTCDecoder on one GPU */

/* ---- lifecycle: replaces DeepSpeech.__init__ / load_model (model.py:293-425, 599-624) */
int dsmi_model_create(const dsmi_model_desc* desc, int device, dsmi_model** out);
/* One call per state_dict entry, reference names ("rnns.0.rnn.weight_ih_l0_reverse", ...);
 * `data` is host float32, row-major, `shape[ndim]`.  Unknown names are ignored
 * (num_batches_tracked). */
int dsmi_model_load_tensor(dsmi_model* m, const char* name, const float* data_host,
                           const int64_t* shape, int ndim);
/* Checks completeness, repacks weights into kernel layouts, uploads.  After this the
 * handle is immutable apart from workspaces. */
int dsmi_model_finalize(dsmi_model* m);
/* Pre-sizes workspaces so that no allocation happens on the timed path for
 * batches <= max_batch of <= max_frames spectrogram frames. */
int dsmi_reserve(dsmi_model* m, int max_batch, int max_frames);
void dsmi_model_destroy(dsmi_model* m);
const char* dsmi_last_error(const dsmi_model* m);

/* ---- DeepSpeech.get_seq_lens (model.py:540-551); pure host arithmetic */
int dsmi_seq_lens(const dsmi_model* m, const int32_t* lens_host, int n, int32_t* out_lens_host);

/* ---- SpectrogramAudioParser (parsers.py:37-72), batched.
 * pcm_dev: B clips back to back, clip b has n_samples_host[b] samples starting at
 * sample offset sum(n_samples_host[:b]); dtype DSMI_PCM_* (float arrays as load_audio returns
 * them, or a WAV file's raw frames: the file never has to be decoded on the host).
 * feat_dev: [B][n_freq][t_stride] float32, frames past a clip's own count are zero.
 * frames_host[b] = 1 + n_samples[b] / hop.  Asynchronous on `stream`.
 * dsmi_frontend_create: DSMI_ERR_INVALID for a window length (sample_rate * window_size) whose direct transform needs more LDS per
 * workgroup (80 bytes per sample of the window) than the device has; the message names both. */
int dsmi_frontend_create(const dsmi_frontend_desc* desc, int device, dsmi_frontend** out);
void dsmi_frontend_destroy(dsmi_frontend* f);
const char* dsmi_frontend_last_error(const dsmi_frontend* f);
int dsmi_features(dsmi_frontend* f, const void* pcm_dev, int pcm_dtype, const int64_t* n_samples_host,
                  int B, float* feat_dev, int t_stride, int32_t* frames_host, void* stream);

/* ---- Sample-rate conversion in front of dsmi_features: AudioData.get_raw_data / get_array_data(convert_rate=...)
 * (resources.py:568-570), batched.  pcm_dev / pcm_dtype / n_samples_host[B] as for dsmi_features (every DSMI_PCM_* type,
 * DSMI_PCM_STEREO included: a WAV file's bytes are resampled as they are); rate_in is the clips' rate, the frontend's
 * sample_rate the rate they are converted to.  out_dev: float64, the resampled clips back to back (clip b at offset
 * sum(n_out_host[:b])), at their integer scale -- what dsmi_features(..., DSMI_PCM_F64, n_out_host, ...) and
 * dsmi_recognize_enqueue_device take; out_capacity is its size in samples, n_out_host[B] receives the clips' new lengths
 * (= dsmi_resample_count).  One launch per call however many clips, asynchronous on `stream`; a clip of 0 samples gives 0.
 *   DSMI_RESAMPLE_POLYPHASE  rational polyphase FIR, the design of scipy.signal.resample_poly's default: with
 *                            up = rate_out / g, down = rate_in / g, half = 10 max(up, down),
 *                                h[m] = sinc(m / max(up, down)) / max(up, down) * kaiser(beta = 5)(m), m = -half .. half, h *= up / sum(h)
 *                                y[j] = sum_k x[k] h[j down - k up]   (x zero outside the clip),   ceil(n up / down) outputs
 *                            float64 taps (made on the host once per rate_in, kept on the handle), float64 sums.
 *   DSMI_RESAMPLE_RATECV     audioop.ratecv(data, width, 1, rate_in, rate_out, None) bit for bit (linear interpolation, no
 *                            low-pass: the reference's own conversion), applied as the reference applies it: after the 8-bit
 *                            bias and the saturating stereo fold, at the file's sample width.  (n - 1) o / i + 1 outputs
 *                            (integer division).  Integer sample types only.
 * rate_in equal to the frontend's rate is no error: both methods then copy the decoded samples.
 * Refused before any launch, with nothing written to out_dev or n_out_host: rate_in <= 0, an unknown method, float PCM with
 * RATECV (DSMI_ERR_INVALID); out_capacity below the sum of the new lengths, a filter of more than DSMI_RESAMPLE_MAX_TAPS taps
 * (16001 -> 16000 has 320 021: admitted; 2.7 MB on the device), rate_in above DSMI_RESAMPLE_MAX_DECIMATION times the
 * frontend's rate (DSMI_ERR_CAPACITY).
 * dsmi_resample_count (host only): the length n samples have after the conversion, < 0 for bad arguments.
 * dsmi_resample_taps (host only): up, down and, when taps_out is not NULL (capacity >= 20 max(up, down) + 1 doubles), the filter
 * h[-half .. half] the polyphase kernel uses; failures are reported by dsmi_frontend_last_error(NULL). */
enum { DSMI_RESAMPLE_POLYPHASE = 0, DSMI_RESAMPLE_RATECV = 1 };
#define DSMI_RESAMPLE_MAX_TAPS (1 << 19)
#define DSMI_RESAMPLE_MAX_DECIMATION 24
int dsmi_resample(dsmi_frontend* f, const void* pcm_dev, int pcm_dtype, const int64_t* n_samples_host, int B, int rate_in,
                  int method, double* out_dev, int64_t out_capacity, int64_t* n_out_host, void* stream);
int64_t dsmi_resample_count(int method, int rate_in, int rate_out, int64_t n);
int dsmi_resample_taps(int rate_in, int rate_out, double* taps_out, int64_t capacity, int* up, int* down);

/* ---- The same conversion for LIVE audio: an utterance that arrives in chunks of any size (no reference counterpart beyond the
 * state argument of audioop.ratecv).  A dsmi_resampler is one utterance in flight.  It belongs to a frontend, whose sample_rate
 * is the rate converted to and which keeps the polyphase filters (shared with dsmi_resample); rate_in, method and pcm_dtype (any
 * DSMI_PCM_*, DSMI_PCM_STEREO included) are fixed at creation, which applies the refusals of dsmi_resample.  Destroy the handles
 * of a frontend before the frontend.
 * The defining property: however the utterance is cut into chunks -- chunks of one sample, empty chunks --, the outputs of its
 * pushes laid end to end are BIT FOR BIT those of one dsmi_resample call over the whole utterance, for both methods, every
 * sample type and equal rates.
 * dsmi_resample_ready (host only): how many outputs are final once the first n_in samples of an utterance are known, < 0 for
 * bad arguments.  POLYPHASE: the j with (j down + half) / up <= n_in - 1, i.e. min(dsmi_resample_count(n_in),
 * max(0, ceil((n_in up - half) / down))) -- the filter looks half / up input samples ahead, under a millisecond.  RATECV:
 * dsmi_resample_count(n_in) (linear interpolation looks no further than the sample it stands on).  Equal rates: n_in.
 * dsmi_resampler_push_many advances n distinct handles of one frontend by one chunk each (1 <= n <= DSMI_RESAMPLE_STREAM_MAX;
 * rates, methods and sample types may differ): pcm_dev[i] holds n_samples[i] >= 0 new samples of session i (frames for stereo;
 * may be NULL for 0).  Session i writes ready(total_in) - emitted outputs -- with is_last[i] the rest, up to
 * dsmi_resample_count(total_in), and then stands at the start of a new utterance -- as float64 at integer scale, the sessions
 * back to back in out_dev (what dsmi_features_stream_many takes); n_out_host[i] receives its count, which is host arithmetic:
 * the call waits for nothing the device does and is asynchronous on `stream` (a frontend's FIRST push sizes the descriptor
 * table and the pinned staging ring for DSMI_RESAMPLE_STREAM_MAX sessions, which waits for the device once; later on the host can
 * only wait for the descriptor copy of the fourth call before, the ring having four slots).  At most one launch per method present (polyphase / ratecv /
 * copy), whatever n.  What a session still needs of its past input (at most 20 max(1, down / up) samples) waits on the device.
 * Refused before any launch, with every handle left exactly as it was and nothing written: n out of range, a handle listed
 * twice, handles of different frontends, a negative count (DSMI_ERR_INVALID), out_capacity below the sum of the outputs
 * (DSMI_ERR_CAPACITY); the error text (dsmi_resampler_last_error(NULL): the thread's last refusal) names the session index.
 * dsmi_resampler_position: samples consumed / outputs written since the utterance began.  dsmi_resampler_reset: a new utterance. */
typedef struct dsmi_resampler dsmi_resampler;
#define DSMI_RESAMPLE_STREAM_MAX 256
int dsmi_resampler_create(dsmi_frontend* f, int rate_in, int method, int pcm_dtype, dsmi_resampler** out);
void dsmi_resampler_destroy(dsmi_resampler* r);
const char* dsmi_resampler_last_error(const dsmi_resampler* r);
int dsmi_resampler_reset(dsmi_resampler* r);
int dsmi_resampler_position(const dsmi_resampler* r, int64_t* n_in, int64_t* n_out);
int64_t dsmi_resample_ready(int method, int rate_in, int rate_out, int64_t n_in);
int dsmi_resampler_push_many(dsmi_resampler* const* rs, int n, const void* const* pcm_dev, const int64_t* n_samples,
                             const int* is_last, double* out_dev, int64_t out_capacity, int64_t* n_out_host, void* stream);

/* ---- Utterances in LIVE audio: Recognizer.listen_stream (Recognizer.py:218-324), the energy gate that cuts a continuous stream
 * into utterances, for up to DSMI_ENDPOINT_MAX sessions per call.  A dsmi_endpointer is one stream in flight.  It belongs to a
 * frontend; everything in dsmi_endpointer_desc is fixed at creation.  Destroy the handles of a frontend before the frontend.
 * The stream is read in buffers of `chunk` samples (16 .. 65536; the stream's final buffer may be shorter).  A buffer's energy is
 * audioop.rms(buffer, 2) = (unsigned) sqrt(S / (double) len), S the sum of its squared samples: the device delivers the exact
 * integer S, the host takes the root with libm.  With spb = chunk / rate (float64), pause_n = ceil(pause_threshold / spb),
 * phrase_n and keep_n (non_speaking_duration) likewise (:239-245):
 *   waiting   the last keep_n buffers are kept, the one just read among them; energy > energy_threshold emits the kept buffers
 *             and starts a phrase with both counts at 0;
 *   phrase    phrase_count += 1; energy > threshold sets pause_count = 0, otherwise pause_count += 1; while pause_count <= pause_n
 *             the buffer is emitted; else the phrase ends: phrase_count -= pause_count, and with phrase_count >= phrase_n the
 *             breaking buffer is emitted with last = 1 (the session stands at the start of a new utterance), otherwise the
 *             breaking buffer is dropped and the session waits again, with nothing kept, inside the same utterance;
 *   end       end_of_stream behaves as the empty read does: the stream's short final buffer is gated like any other, then a waiting
 *             session emits what it keeps, and a segment of 0 samples closes the utterance with last = 1.
 * timeout and phrase_time_limit are not taken over.
 * Sample types: DSMI_PCM_I16, I16 | STEREO (the saturating fold of audioop.tomono(.., 1, 1), as SpeechFileStream.read applies it),
 * F32 and F64.  Float samples enter S as llrint(x) saturated to int16 and are FORWARDED UNCHANGED.  U8, I24 and I32 are refused at
 * creation (DSMI_ERR_INVALID): the reference's 8-bit rms reads the unsigned bytes as signed, and sums of squared 24/32-bit samples
 * are not exact in float64, so neither could be matched exactly.
 * dsmi_endpoint_counts (host only): {pause_n, phrase_n, keep_n} of a desc, < 0 for a desc that create would refuse.
 * dsmi_endpoint_gate (host only): the state machine over n_buffers buffers given by their sums S[i] and sample counts len[i].
 * state4 = {phase (0 waiting, 1 phrase), kept, phrase_count, pause_count}, all 0 at the start of a stream, is read and updated.
 * Events (first_buffer, n_buffers, last) are appended: first_buffer counts from the run's first buffer and is negative where the
 * event begins in the buffers kept from earlier runs.  What the reference yields one buffer at a time is joined: an event is a run
 * of consecutive buffers, ended by a last mark, a dropped buffer or the end of the run.  Returns the number of events (at most
 * n_buffers + 1 ; only max_events are stored), < 0 for bad arguments.  energies (optional) receives the n_buffers energies.
 * dsmi_endpointer_push_many hands n distinct handles of one frontend their next samples (1 <= n <= DSMI_ENDPOINT_MAX; chunks,
 * thresholds and sample types may differ): pcm_dev[i] holds n_samples[i] >= 0 new samples of session i (frames for stereo; may be
 * NULL for 0); end_of_stream[i] ends the stream after them.  Kernel 1 sums the squares of every buffer that is complete now (one
 * wave per buffer) into pinned host memory; one synchronisation of `stream`; the host runs dsmi_endpoint_gate for every session;
 * kernel 2 writes the emitted segments back to back to out_dev, in event order (session by session), as float64 at integer scale
 * -- what dsmi_features_stream_many(DSMI_PCM_F64) and a polyphase dsmi_resampler take -- and each session's retained tail: the
 * kept buffers of a waiting session and the incomplete buffer at the end of the push, at most (keep_n + 1) chunk samples.
 * seg_session / seg_len / seg_last [max_segments] receive the segments, *n_segments their number.  energies_host (optional)
 * receives the energy of every buffer gated in this call, session by session: session i gates
 * (consumed + n_samples) / chunk - consumed / chunk buffers, and one more at end_of_stream when a short final buffer remains.
 * Two launches and one synchronisation per call whatever n (no first launch and no synchronisation for a call that completes no
 * buffer; the second launch is repeated per 65535 copies, which takes a push of tens of thousands of buffers).  No device or pinned
 * memory is allocated after a frontend's first push unless one call gates more than 16 buffers per session of 256 (the tables then
 * grow, which waits for the device); the call's host-side scratch (the plan, the tables' host images, the events) is ordinary
 * heap memory taken and released per call.  More than 2^27 buffers in one call are refused like the other bad arguments.
 * The defining property: however a stream is cut into pushes -- pushes of one sample, empty pushes, a push that spans three
 * utterances --, the segments laid end to end and the positions of the last marks are BIT FOR BIT those of one push of the whole
 * stream with end_of_stream.  Where a cut falls may split or join segments, never change the samples or the marks.
 * Refused before any launch, with every handle left exactly as it was and nothing written: n out of range, a handle listed twice,
 * handles of two frontends, a negative count, samples after a session's end_of_stream without a reset (DSMI_ERR_INVALID);
 * out_capacity below the worst case sum(held_i + n_samples_i), or max_segments below the worst case, the sum over the sessions
 * that gate b_i > 0 buffers or end of b_i + 1 (DSMI_ERR_CAPACITY).  The error text (dsmi_endpointer_last_error(NULL): the thread's
 * last refusal) names the session index.
 * dsmi_endpointer_position: samples consumed since the stream began, utterances closed, samples held on the device.
 * dsmi_endpointer_reset: a fresh stream. */
typedef struct dsmi_endpointer dsmi_endpointer;
#define DSMI_ENDPOINT_MAX 256
typedef struct {
    int32_t chunk;                  /* samples per buffer (source.chunk), 16 .. 65536            */
    int32_t rate;                   /* the source's sampling rate                               */
    int32_t pcm_dtype;              /* DSMI_PCM_I16, I16 | STEREO, F32, F64                      */
    double  energy_threshold;       /* Recognizer.energy_threshold (1000)                        */
    double  pause_threshold;        /* seconds (0.8)                                             */
    double  phrase_threshold;       /* seconds (0.3)                                             */
    double  non_speaking_duration;  /* seconds (0.35); pause_threshold >= non_speaking_duration >= 0 */
} dsmi_endpointer_desc;
int dsmi_endpoint_counts(const dsmi_endpointer_desc* desc, int64_t* counts3);
int64_t dsmi_endpoint_gate(double energy_threshold, int64_t pause_n, int64_t phrase_n, int64_t keep_n, int64_t* state4,
                           const uint64_t* S, const int64_t* len, int64_t n_buffers, int end_of_stream, int64_t* ev_first,
                           int64_t* ev_count, int32_t* ev_last, int64_t max_events, uint32_t* energies);
int dsmi_endpointer_create(dsmi_frontend* f, const dsmi_endpointer_desc* desc, dsmi_endpointer** out);
void dsmi_endpointer_destroy(dsmi_endpointer* e);
const char* dsmi_endpointer_last_error(const dsmi_endpointer* e);
int dsmi_endpointer_reset(dsmi_endpointer* e);
int dsmi_endpointer_position(const dsmi_endpointer* e, int64_t* n_in, int64_t* n_utterances, int64_t* n_held);
int dsmi_endpointer_push_many(dsmi_endpointer* const* es, int n, const void* const* pcm_dev, const int64_t* n_samples,
                              const int* end_of_stream, double* out_dev, int64_t out_capacity, int32_t* seg_session,
                              int64_t* seg_len, int32_t* seg_last, int max_segments, int* n_segments, uint32_t* energies_host,
                              void* stream);

/* ---- InferenceSpectrogramAudioParser.parse_audio (parsers.py:102-164), the arithmetic half: STFT of the
 * samples WITHOUT centre padding (librosa.stft(center=False), :137-138: 1 + (n - n_fft)/hop frames), log1p|.|,
 * then the adaptive normalisation of :146-161.  state3 = {input_mean, input_std, alpha} is read and updated
 * exactly as the parser's attributes are (alpha += 0.1; running mean/std halved with the chunk's np.mean /
 * np.std; while alpha < 1 they are mixed with the NST dataset statistics 5.492418704733003 /
 * 1.7552755216970917, :89-94).  The sample bookkeeping of :112-133 (hop carry-over) stays with the caller.
 * feat_dev [n_freq][t_stride]; *frames_host = frames written.  Synchronous (the statistics pass through
 * the host).  Start an utterance with state3 = {0, 0, 0} (parser.reset(), :166-170). */
/* Host only.  load_audio hands recognize() float64 samples (reference resources.py:640) that are, for every audio FILE, integers in
 * int16's range: such a clip travels to the device as int16 -- a quarter of the bytes, the same features bit for bit (dsmi_features
 * widens to float64 exactly).  Returns 1 when every one of the n samples is an integer in [-32768, 32767] and dst holds them, 0
 * when one is not (dst is then unspecified and the caller uploads the float64 samples).  Used by the staging of
 * dsmi_recognize_enqueue and of the Python pipeline. */
int dsmi_pack_pcm_i16(const double* src, int64_t n, int16_t* dst);
/* Staged clips -> device memory by a KERNEL that reads the pinned host buffer over the bus (src_pinned: hipHostMalloc'ed / pinned by
 * the caller's framework, i.e. mapped into the device's address space; bytes a multiple of 2), asynchronous on `stream`.  The
 * batch pipeline uploads with it instead of hipMemcpyAsync: the runtime hands a copy to a DMA engine, and the first copies a
 * process's streams give the engines hold the calling thread for 6-12 ms each -- well into a process's second call
 * (profiles/r06_second_call_stall.txt).  device: where dst_dev lives. */
int dsmi_upload(int device, void* dst_dev, const void* src_pinned, int64_t bytes, void* stream);
int dsmi_features_stream(dsmi_frontend* f, const void* pcm_dev, int pcm_dtype, int64_t n_samples, double* state3,
                         float* feat_dev, int t_stride, int32_t* frames_host, void* stream);
/* The streaming parser for n sessions in one pass: their chunks back to back in pcm_dev (n_samples[i] samples each),
 * features to feat_dev [n][n_freq][t_stride], frames_host[i] = session i's frame count, and session i's running
 * statistics state3[3*i .. 3*i+2] updated.  One STFT launch, one statistics launch, one host synchronisation, one
 * normalise launch; session i's result equals its own dsmi_features_stream call. */
int dsmi_features_stream_many(dsmi_frontend* f, const void* pcm_dev, int pcm_dtype, const int64_t* n_samples, int n,
                              double* state3, float* feat_dev, int t_stride, int32_t* frames_host, void* stream);

/* ---- Chunked unidirectional inference: DeepSpeech(streaming_inference_model=True).streaming_forward
 * (model.py:517-537) with the state MaskConvStream (:156-201), BatchRNNStream (:204-238) and LookaheadStream
 * (:241-283) carry between calls.  One dsmi_stream = one utterance in flight (B = 1) on a unidirectional
 * 2-conv model (the only streaming shape the reference can run: streaming_init, :427-494); a model serves any
 * number of streams.  feat_dev [n_freq][T] float32 (one chunk of the streaming parser's output);
 * probs_dev [T_out_cap][n_labels].  *T_out = frames written: 0 on the first pass (is_first), when the
 * lookahead only buffers (streaming_forward returns None, :529-530).  is_last flushes the lookahead with its
 * right padding and clears all carried state.  Asynchronous on `stream`.  A refused call (DSMI_ERR_INVALID, DSMI_ERR_CAPACITY)
 * changes nothing; after DSMI_ERR_HIP the handle's carried state is undefined until dsmi_stream_reset. */
typedef struct dsmi_stream dsmi_stream;
int dsmi_stream_create(dsmi_model* m, dsmi_stream** out);
void dsmi_stream_destroy(dsmi_stream* s);
const char* dsmi_stream_last_error(const dsmi_stream* s);
int dsmi_stream_reset(dsmi_stream* s);
int dsmi_stream_forward(dsmi_stream* s, const float* feat_dev, int T, int is_first, int is_last, float* probs_dev,
                        int T_out_cap, int32_t* T_out, void* stream);
/* Advances n sessions of ONE model by one chunk each in one batched pass whose launch count does not depend on n
 * (1 <= n <= DSMI_STREAM_MANY_MAX).  streams[i] are distinct handles of the same dsmi_model; feat_dev[i] is session i's
 * chunk [n_freq][T[i]] float32 on the device; is_first[i] / is_last[i] as for dsmi_stream_forward.  Session i's
 * probabilities go to probs_dev + i * T_out_cap * n_labels (frames past T_out[i] of its slot are scratch), and T_out[i]
 * receives its frame count (0 while its lookahead is still buffering).  Each handle is left exactly as the same chunk
 * through dsmi_stream_forward would leave it, so a session may alternate freely between the two calls.  Either every
 * session advances or the call is refused with no session's state changed; the error text (dsmi_stream_last_error(NULL))
 * names the session index.  Returns when the pass is complete (the caller's stream is synchronised). */
#define DSMI_STREAM_MANY_MAX 256
int dsmi_stream_forward_many(dsmi_stream* const* streams, int n, const float* const* feat_dev, const int* T,
                             const int* is_first, const int* is_last, float* probs_dev, int T_out_cap, int32_t* T_out,
                             void* stream);

/* ---- Offline long-form segmentation: the energy gate of
 * example_scripts/video_transcribe_simulation.py:68-143 over one recording.
 * Hop i covers samples [i*step, (i+1)*step) for every i with (i+1)*step < n_samples (:94); its energy is
 * sqrt(sum(x*x)/step) in float64 (:100), summed in numpy's pairwise order so that comparisons with
 * energy_threshold fall exactly as they do in the script.  A phrase starts at the first hop above the
 * threshold, two hops early when that is not negative (:103-113), ends once more than pause_hops
 * consecutive hops stay at or below it (:119-128), and is reported when it held more than phrase_hops
 * hops apart from that pause (:131-132).  A phrase still open at the end of the audio is dropped, as in
 * the script.  step must be 128 * 2^k.  seg_start/seg_end_host[max_segments] receive sample ranges
 * [start, end); *n_segments the number found (DSMI_ERR_CAPACITY if more than max_segments).
 * energies_host (optional, one float64 per hop) receives the hop energies.  Synchronous. */
int dsmi_segment(dsmi_frontend* f, const void* pcm_dev, int pcm_dtype, int64_t n_samples, int step,
                 double energy_threshold, int pause_hops, int phrase_hops,
                 int64_t* seg_start_host, int64_t* seg_end_host, int max_segments, int* n_segments,
                 double* energies_host, void* stream);

/* ---- DeepSpeech.forward (model.py:496-515), eval mode.
 * feat_dev [B][1][n_freq][T] float32 (T = max frames, zero past each clip's length),
 * lens_host[B] sorted descending.  probs_dev [B][T_out][n_labels] float32 softmax
 * probabilities where T_out = seq_lens(T); out_lens_host[B]. */
int dsmi_forward(dsmi_model* m, const float* feat_dev, const int32_t* lens_host, int B, int T,
                 float* probs_dev, int32_t* out_lens_host, void* stream);
/* dsmi_forward is asynchronous on `stream`; dsmi_forward_status blocks until the handle's OLDEST dsmi_forward whose
 * status has not been collected yet has finished, and says whether its results are valid (the reference's forward is
 * synchronous and cannot fail this way: torch's CPU kernels do not depend on co-residency).  Call it once per forward,
 * in order, before consuming that forward's probs_dev; its feat_dev, probs_dev and stream must still be alive.  Up to 4
 * forwards may be in flight uncollected (a pipelining caller enqueues batch i+1 before collecting batch i).
 *   DSMI_OK          results valid.
 *   DSMI_RECOMPUTED  a hand-off wait inside the persistent recurrent kernel timed out (not all of its workgroups were
 *                    resident: another kernel or process occupied compute units).  The SAME batch has been recomputed
 *                    with one launch per time step into the same probs_dev before this call returned: results valid
 *                    now, and the handle keeps using the per-step path.  dsmi_last_error() holds a description.
 *   < 0              the recompute itself failed.
 * Uncollected forwards that finished well are forgotten by the next dsmi_forward; one that finished with a timeout
 * makes the next dsmi_forward fail with DSMI_ERR_TIMEOUT (its results were invalid and may have been consumed). */
int dsmi_forward_status(dsmi_model* m);
/* 1 when the handle's oldest uncollected dsmi_forward has finished on the device (dsmi_forward_status would not block), 0 when
 * it is still running, < 0 on error; never blocks.  For a host that keeps several handles busy and refills whichever
 * finishes first (no reference counterpart). */
int dsmi_forward_ready(dsmi_model* m);
/* Tells the handle how many batches the caller keeps in flight on this device (each on its own handle and stream).
 * 1 (default): kernels chosen for the latency of one batch (one 16-clip tile per workgroup, the whole device).  2: the
 * recurrent layers use the paired-tile variant (a workgroup carries both tiles of a 17..32-clip batch: 100 CUs for
 * BASELINE's 5 x BiGRU 800) where the shape allows it, so that the two batches' recurrent layers run side by side on
 * disjoint halves of the chip.  Results are the same either way (within the parity bound). */
int dsmi_model_set_inflight(dsmi_model* m, int batches);
/* How many ring windows (rnn_persist_ring*.hip: H / 32 workgroups per direction each, 50 CUs for 5 x BiGRU 800) the recurrent layers of
 * this handle's NEXT forwards take side by side.  0 (default): what set_inflight implies -- one window with batches in flight, as
 * many as the batch has tile pairs (up to four) for a lone batch.  2: a caller that knows that only two forwards will share the
 * chip (the last forwards of a short call) gives each two windows of half the tiles: 2.7 instead of 3.2 ms per 64-clip layer.
 * Shapes the ring kernels do not take ignore it.  Results are the same either way (within the parity bound). */
int dsmi_model_set_ring_windows(dsmi_model* m, int windows);
/* Number of batches / layers this handle had to recompute after a hand-off timeout (0 in normal operation). */
int dsmi_recompute_count(const dsmi_model* m);

/* Stage-level entry points (same arithmetic as inside dsmi_forward), used by the
 * parity tests against the reference's MaskConv (model.py:65-81) and BatchRNN
 * (model.py:114-122) golden vectors.
 * conv_out_dev: [B][C_out*F_out][T_out] float32.
 * rnn layer: x_dev/y_dev are [T][B][I] / [T][B][H] float32 (reference T x N x H). */
int dsmi_conv_stack(dsmi_model* m, const float* feat_dev, const int32_t* lens_host, int B, int T,
                    float* conv_out_dev, void* stream);
int dsmi_rnn_layer(dsmi_model* m, int layer, const float* x_dev, const int32_t* out_lens_host,
                   int B, int T_out, float* y_dev, void* stream);
/* The output head by itself (model.py:508-514): x_fwd_dev / x_rev_dev are the last recurrent layer's outputs per direction,
 * dense [T_out][B][H] float32; x_rev_dev is required exactly when the model is bidirectional (NULL otherwise).  Unidirectional
 * models run the Lookahead + Hardtanh first.  probs_dev: [B][T_out][n_labels] float32.  Bad arguments are refused before any
 * launch; the call returns when the result is there. */
int dsmi_head(dsmi_model* m, const float* x_fwd_dev, const float* x_rev_dev, int B, int T_out,
              float* probs_dev, void* stream);

/* ---- Decoder.__init__ (decoder.py:35-43): labels as n_labels UTF-8 strings (labels may be
 * multi-byte, e.g. the Danish letters), blank_index as DanSpeechRecognizer passes it
 * (labels.index('_'), DanSpeechRecognizer.py:92,94). */
int dsmi_decoder_create(int device, const char* const* labels_utf8, int n_labels, int blank_index,
                        dsmi_decoder** out);
void dsmi_decoder_destroy(dsmi_decoder* d);
const char* dsmi_decoder_last_error(const dsmi_decoder* d);

/* ---- GreedyDecoder.decode (decoder.py:183-198 + 151-181).
 * probs_dev [B][T_out][n_labels]; sizes_host[B] or NULL (= T_out for all).
 * ids_host/offsets_host: [B][T_out] int32, first n_out_host[b] entries valid.  Synchronises. */
int dsmi_greedy(dsmi_decoder* d, const float* probs_dev, const int32_t* sizes_host, int B, int T_out,
                int32_t* ids_host, int32_t* offsets_host, int32_t* n_out_host, void* stream);
/* The same call in two halves for a host that keeps batches in flight (no reference counterpart: GreedyDecoder.decode is a
 * host loop, decoder.py:166-198).  _enqueue launches the kernel and the copies of its results on `stream` -- behind the
 * dsmi_forward that writes probs_dev -- and returns at once; _collect waits for them and fills the arrays of dsmi_greedy.
 * One decode per handle at a time. */
int dsmi_greedy_enqueue(dsmi_decoder* d, const float* probs_dev, const int32_t* sizes_host, int B, int T_out, void* stream);
int dsmi_greedy_collect(dsmi_decoder* d, int32_t* ids_host, int32_t* offsets_host, int32_t* n_out_host);

/* ---- measurement hooks (no reference counterpart; SURVEY 5 "tracing/profiling": none).
 * level 0: off.  level 1: per-stage hipEvents around the last dsmi_forward (synchronises).
 * level 2: sampled launches of each kernel kind are dispatched with their own begin/end
 * timestamps (hipExtLaunchKernelGGL), fully asynchronous; read back with dsmi_kernel_stats.
 * Sampled = every launch of the recurrent kinds (6, 10), every fourth of the others.
 * stage for dsmi_stage_time_us: 0 conv, 2 input GEMMs + recurrent steps, 3 head, 4 total. */
int dsmi_set_profiling(dsmi_model* m, int level);
/* kind: 0 stft, 1 conv1, 2 conv2, 3 conv3, 4 layer-0 input GEMM, 5 input GEMM (layers >= 1),
 * 6 recurrent step (per-step path), 7 head, 8 greedy, 9 beam, 10 persistent recurrent layer.  launches = dispatches since the last reset,
 * samples = how many of them were timed, avg_us = mean duration of the timed ones,
 * flops/bytes_per_launch = algorithmic work (SURVEY 8d formulas) averaged over all launches. */
int dsmi_kernel_stats(dsmi_model* m, int kind, int64_t* launches, int64_t* samples, double* avg_us,
                      double* flops_per_launch, double* bytes_per_launch);
int dsmi_reset_kernel_stats(dsmi_model* m);
/* Diagnostics build of the recurrent step kernel: per-wave phase timestamps (100 MHz
 * s_memrealtime ticks) of the launch for `step` of `layer`; stamps_host[D*nwg][8][8]. */
int dsmi_debug_persist_stamps(dsmi_model* m, int layer, int B, int T_out, uint64_t* stamps_host, int64_t n_words);
int dsmi_debug_step_stamps(dsmi_model* m, int layer, int B, int T_out, int step, uint64_t* stamps_host,
                           int64_t n_words);
/* Which kernels ran: the launches the handle's LAST recurrent layer (of dsmi_forward, dsmi_rnn_layer or a recompute) actually made,
 * after any fallback that followed a launcher's refusal, as text: "x16|" or "x8|" (the column order of the x-projection), then per
 * launch "kernel at n nwin gate slot0 nslots cus ticket part;" with kernel one of steps, persist8, p16w8, p16w4, duo, ring8, ring4
 * (csrc/rnn_plan.h: RnnLaunch; the format of tools/asan/host_fuzz.cpp rnnplan).  Returns the number of launches the layer made (0
 * and an empty string before the first layer); the text holds the first eight of them.  Recording allocates nothing.
 * dsmi_stream_forward and dsmi_stream_forward_many record their recurrent layers here too, one launch per layer: "persist8 0 1 1 lane
 * 0 4 <workgroups> 0 1;" for the batched pass's carried-state launch, "steps ..." otherwise (a shape the persistent kernel does not
 * take, DSMI_RNN_MODE=steps, every single-session call, and the recomputation of a timed-out pass).
 * DSMI_ERR_INVALID: null argument or a buffer too small (1400 bytes hold any answer). */
int dsmi_debug_last_rnn_plan(const dsmi_model* m, char* buf, int64_t capacity);
/* The x-projection the handle's LAST recurrent layer ran on (the GEMM's output, bias included, in the column order the layer's
 * kernels read): rows [T_out * B] of *cols floats, copied to xp_host once the device is idle; *workgroups: how many workgroups that
 * GEMM was launched with (one per tile, rounded up to eight, in the static order; at most two per CU by demand).  For tests that
 * compare two forms of the GEMM bit for bit and must know that two forms ran.  DSMI_ERR_INVALID: null argument, no layer yet, or
 * capacity (in floats) below rows * cols. */
int dsmi_debug_xproj(dsmi_model* m, float* xp_host, int64_t capacity, int32_t* rows, int32_t* cols, int32_t* workgroups);
/* How many workgroups each conv layer's LAST launch on the handle had: workgroups[l] for layer l (one per tile in the static order;
 * min(tiles, 2 x CUs) by demand; 0: the layer has not run, or ran on the fp32 kernel).  Host bookkeeping, no device call.  Returns
 * the number of conv layers; DSMI_ERR_INVALID: null argument or capacity below it. */
int dsmi_debug_conv_workgroups(const dsmi_model* m, int32_t* workgroups, int32_t capacity);
/* Experiments build of the library, with DSMI_DEBUG_TILE_STAMPS=1: where the XCDs ended inside each of the process's first 4096
 * launches of the x-projection GEMM, 32 words per launch (csrc/gemm.hip: kTileStampWords; tools/exp/dense_tile_spread.py prints
 * them).  Returns the number of launches copied to stamps_host (at most n_words / 32); the product library records nothing: 0. */
int dsmi_debug_dense_stamps(uint64_t* stamps_host, int64_t n_words);
double dsmi_stage_time_us(const dsmi_model* m, int stage);
/* Kernel launches the last dsmi_forward issued for stage 2 (recurrent steps) and their
 * summed algorithmic FLOPs (SURVEY 8d formula, recurrent part), for roofline maths. */
int dsmi_last_forward_stats(const dsmi_model* m, int64_t* n_step_launches, double* step_flops,
                            double* total_flops);

/* ---- BeamCTCDecoder (decoder.py:91-144): what ctcdecode.CTCBeamDecoder(labels, lm_path, alpha,
 * beta, cutoff_top_n, cutoff_prob, beam_width, num_processes, blank_index).decode(probs, sizes)
 * does for the reference (third-party, not in the reference tree; restated in oracle/beam.py).
 * dsmi_decoder_set_lm: lm_path = an n-gram model of order <= 6 -- a KenLM binary (.klm, what the reference's
 * language_models.* factories return, danspeech/language_models/dsl_3gram.py:16-20: data structures `probing` and
 * `trie`, unquantised) or ARPA text -- or NULL/"" for none; the file type is told by its first bytes.
 * dsmi_beam outputs, all host: tokens/tsteps [B][beam][T_out] int32 (token ids and the frame
 * of each token's strongest emission), lens [B][beam], scores [B][beam] (ctcdecode's
 * "-approx_ctc", lower is better; beams are ordered best first).  Synchronises. */
int dsmi_decoder_set_lm(dsmi_decoder* d, const char* lm_path, double alpha, double beta);
int dsmi_beam(dsmi_decoder* d, const float* probs_dev, const int32_t* sizes_host, int B, int T_out,
              int beam_width, int cutoff_top_n, double cutoff_prob, int32_t* tokens_host,
              int32_t* tsteps_host, int32_t* lens_host, float* scores_host, void* stream);
/* The two halves of dsmi_beam, for callers that keep the GPU busy meanwhile (ctcdecode decodes on a host thread pool while
 * the caller waits; here the search itself is a kernel): dsmi_beam_enqueue launches the search asynchronously on `stream`
 * (probs_dev must stay valid until the collect); dsmi_beam_collect waits for it, copies the results (on that stream, into
 * pinned memory of the handle) and fills the arrays.  One search per decoder handle at a time.
 * dsmi_decoder_beam_stats: how often the last collected search left its fast path, summed over the batch -- counts4 =
 * {dormant prefixes that re-entered the beam, node-pool hops walked for them, exact rankings of a threshold bin from the
 * list, exact rankings against all candidates}; diagnostics for the tests and profiles, no reference counterpart. */
int dsmi_beam_enqueue(dsmi_decoder* d, const float* probs_dev, const int32_t* sizes_host, int B, int T_out,
                      int beam_width, int cutoff_top_n, double cutoff_prob, void* stream);
int dsmi_beam_collect(dsmi_decoder* d, int32_t* tokens_host, int32_t* tsteps_host, int32_t* lens_host, float* scores_host);
int dsmi_decoder_beam_stats(const dsmi_decoder* d, int32_t* counts4);
/* Diagnostics: phase boundaries of the last collected search's first utterance, 64 frames from the middle of the clip x 8 stamps
 * (100 MHz ticks; 0 = frame start, 1..6 = after the frame's six barriers); tools/beam_stamps.py prints the anatomy. */
int dsmi_debug_beam_stamps(const dsmi_decoder* d, uint64_t* stamps_host, int64_t n_words);

/* ---- Resumable beam search: one utterance's CTC prefix beam search carried from one chunk of probabilities to the next, so
 * that a streaming caller pays for each chunk's frames once and can read the best hypotheses of the whole utterance so far
 * after every chunk.  A dsmi_beam_stream is bound to one dsmi_decoder and searches with that decoder's language model, alpha
 * and beta and the beam_width / cutoff_top_n / cutoff_prob given here.  Its state and node pool are device buffers of its own;
 * it never touches the decoder's offline-search workspace nor a pending dsmi_beam_enqueue.  A decoder serves any number of
 * streams; destroy every stream of a decoder before the decoder.  dsmi_decoder_set_lm on the decoder retires its streams:
 * their later advances and collects are refused (create new ones).  dsmi_beam_stream_reset starts a new utterance.
 *
 * dsmi_beam_stream_advance_many advances n distinct streams of one decoder, with equal beam settings, in ONE launch on
 * `stream` (1 <= n <= DSMI_BEAM_STREAM_MANY_MAX): stream i by frames[i] >= 0 rows of probs_dev[i] (device, [frames[i]][n_labels]
 * float32, the softmax output; may be NULL when frames[i] = 0).  With n_best > 0 (<= beam_width) it also produces each
 * stream's n_best best hypotheses over ALL its frames so far, exactly those dsmi_beam returns first for the concatenated
 * probabilities (timesteps count from the utterance's first frame); they wait in the handle for
 * dsmi_beam_stream_collect_many, and until then the stream refuses to advance.  Either every stream advances or the call is
 * refused with no stream's state changed (bad arguments, a handle listed twice, handles of different decoders or beam
 * settings, a collect pending, a retired stream); the error text (dsmi_beam_stream_last_error(NULL)) names the stream index.
 * Returns when the launch is complete (`stream` is synchronised).
 *
 * dsmi_beam_stream_collect_many hands the pending hypotheses of n streams over in dsmi_beam's layouts cut to n_best:
 * tokens / tsteps [n][n_best][T_stride], lens [n][n_best], scores [n][n_best] (ctcdecode's -approx_ctc), counts [n] (beams
 * present: min(beams in the search, n_best); rows past it have length 0).  Refused with nothing written when a stream has none
 * pending, was advanced with another n_best, or holds a hypothesis longer than T_stride. */
typedef struct dsmi_beam_stream dsmi_beam_stream;
#define DSMI_BEAM_STREAM_MANY_MAX 4096
int dsmi_beam_stream_create(dsmi_decoder* d, int beam_width, int cutoff_top_n, double cutoff_prob, dsmi_beam_stream** out);
void dsmi_beam_stream_destroy(dsmi_beam_stream* s);
const char* dsmi_beam_stream_last_error(const dsmi_beam_stream* s);
int dsmi_beam_stream_reset(dsmi_beam_stream* s);
int dsmi_beam_stream_frames(const dsmi_beam_stream* s, int64_t* frames);
int dsmi_beam_stream_advance_many(dsmi_beam_stream* const* streams, int n, const float* const* probs_dev, const int32_t* frames,
                                  int n_best, void* stream);
int dsmi_beam_stream_collect_many(dsmi_beam_stream* const* streams, int n, int n_best, int T_stride, int32_t* tokens_host,
                                  int32_t* tsteps_host, int32_t* lens_host, float* scores_host, int32_t* counts_host);

/* ---- CTC forced alignment (no reference counterpart): the most probable frame-level CTC path of a transcript the caller
 * already has, through the probabilities dsmi_forward wrote.  The decoder's language model plays no part.
 * probs_dev [B][T_out][n_labels]; sizes_host[B] frames per clip (NULL = T_out for all); targets_host [B][L_stride] label ids,
 * clip b's first target_lens_host[b] valid (never the blank; 0 tokens is legal: the path is all blanks).
 * Clip b with L tokens has S = 2L + 1 states: blank, t_1, blank, t_2, ..., blank.  With lp(t, c) = logf(fmaxf(p, FLT_MIN))
 * accumulated in float32 over frames in order,
 *     alpha_t(s) = max(alpha_{t-1}(s), alpha_{t-1}(s-1), alpha_{t-1}(s-2) [only if s is a token state and
 *                  label(s) != label(s-2)]) + lp(t, label(s)),   alpha_0 = {lp(0, blank), lp(0, t_1), -inf, ...}.
 * Tie rule (part of the contract): a state's predecessor on equal alpha is s, then s-1, then s-2; the path ends in the
 * trailing blank S-1 unless alpha(S-2) (the last token) is strictly larger.
 * Outputs: spans_host [B][L_stride][2] = frames [start, end) the path spends in token k's state; token_probs_host
 * [B][L_stride] = the float32 mean of p(t, label_k) over those frames (summed in frame order); path_logp_host [B] = the
 * path's sum of lp (natural log); status_host [B] = 0 aligned, 1 infeasible (L + #{k : t_k == t_{k+1}} > frames: path_logp
 * = -inf).  Rows past target_lens[b] and the rows of infeasible clips are 0.
 * Refused with nothing written (DSMI_ERR_INVALID; DSMI_ERR_CAPACITY for L_stride above the limit): B <= 0, T_out <= 0,
 * sizes[b] outside 0 .. T_out, target_lens[b] outside 0 .. L_stride, L_stride > DSMI_ALIGN_MAX_TOKENS, a target id that is
 * the blank or >= n_labels.  The limit comes from LDS: two alpha rows of S floats per clip.  Synchronises `stream`. */
#define DSMI_ALIGN_MAX_TOKENS 4096
int dsmi_align(dsmi_decoder* d, const float* probs_dev, const int32_t* sizes_host, int B, int T_out,
               const int32_t* targets_host, const int32_t* target_lens_host, int L_stride,
               int32_t* spans_host, float* token_probs_host, float* path_logp_host, int32_t* status_host,
               void* stream);

/* ---- Long-form CTC forced alignment (no reference counterpart): dsmi_align for ONE recording that is too long for it -- a
 * sitting, a lecture, a film with its subtitles -- whose probabilities are the softmax rows of all its phrases, concatenated in
 * time order, and whose transcript is the whole text.  Where each sentence lies is what the alignment finds ("CTC
 * segmentation").  The decoder's language model plays no part.
 * probs_dev [T][n_labels] float32; targets_host [L] label ids, never the blank (L = 0 is legal: the path is all blanks).
 * The recurrence (the contract) is dsmi_align's, word for word: S = 2L + 1 states, blank, t_1, blank, ..., blank; lp(t, c) =
 * logf(fmaxf(p, FLT_MIN)), accumulated in float32 over frames in order;
 *     alpha_t(s) = max(alpha_{t-1}(s), alpha_{t-1}(s-1), alpha_{t-1}(s-2) [only if s is a token state and
 *                  label(s) != label(s-2)]) + lp(t, label(s)),   alpha_0 = {lp(0, blank), lp(0, t_1), -inf, ...};
 * a state's predecessor on equal alpha is s, then s-1, then s-2; the path ends in the trailing blank S-1 unless alpha(S-2)
 * (the last token) is strictly larger.
 * One addition: a FREE blank state costs 0 at every frame it holds, frame 0 included (its lp(t, blank) is replaced by 0.0f in
 * alpha_0 and in the recurrence).  State 0 is free when lead_free is 1, state S-1 when tail_free is 1; with L = 0 the single
 * state is free when either is.  So audio before the transcript starts, or after it ends, costs nothing.  The tie rules are
 * unchanged.
 * Outputs, as dsmi_align's for one clip: spans_host [L][2] = frames [start, end) the path spends in token k's state;
 * token_probs_host [L] = the float32 mean of p(t, label_k) over them (summed in frame order); path_logp_host [1]; status_host
 * [1] = 0 aligned, 1 infeasible (L + #{k : t_k == t_{k+1}} > T: path_logp = -inf, the rows are 0).  With both flags 0 and L <=
 * DSMI_ALIGN_MAX_TOKENS every output is bit-identical to dsmi_align's of the same clip: each alpha is formed from the same
 * operands by the same additions, however the trellis is tiled.
 * How it runs: the trellis is cut into frame tiles of F frames and state tiles of W states (dsmi_align_long_plan).  Per frame
 * tile one launch, one workgroup per state tile, which reloads alpha of the tile's first frame on its states and the 2F to their
 * left, runs the F frames in LDS and stores its own states' last row: one float32 row of S per frame tile stays on the handle
 * ("checkpoint rows": frame tiles + 1 of them), and no backpointers.  One more launch walks the path back tile by tile,
 * recomputing at most 2F + 1 states of each; a last one forms the token means.  No launch signals between its workgroups.
 * Refused with nothing written: DSMI_ERR_INVALID for T <= 0, L < 0, a flag outside 0 / 1, a target that is the blank or not a
 * label, a NULL d, probs_dev, path_logp_host or status_host, or with L > 0 a NULL targets_host, spans_host or
 * token_probs_host; DSMI_ERR_CAPACITY, the limit named in the message, for L > DSMI_ALIGN_LONG_MAX_TOKENS, T >
 * DSMI_ALIGN_LONG_MAX_FRAMES or checkpoint rows above DSMI_ALIGN_LONG_MAX_WORKSPACE bytes.  What the numbers alone refuse is
 * refused before any array is read.  The workspace lives on the handle and grows on demand.  Synchronises `stream`.
 * dsmi_align_long_plan (host only, no handle): the geometry the call will use, info = {states per state tile W, frames per frame
 * tile F, state tiles = ceil(S / W), frame tiles = ceil((T - 1) / F), checkpoint rows, their bytes = rows * S * 4}.  Returns
 * DSMI_OK, or the code with which dsmi_align_long would refuse T and L on the numbers; DSMI_ERR_INVALID for a NULL info. */
#define DSMI_ALIGN_LONG_MAX_TOKENS (1 << 20)
#define DSMI_ALIGN_LONG_MAX_FRAMES (1 << 22)
#define DSMI_ALIGN_LONG_MAX_WORKSPACE (4ull << 30)
int dsmi_align_long(dsmi_decoder* d, const float* probs_dev, int T, const int32_t* targets_host, int L,
                    int lead_free, int tail_free, int32_t* spans_host, float* token_probs_host, float* path_logp_host,
                    int32_t* status_host, void* stream);
int dsmi_align_long_plan(int T, int L, int64_t* info);

/* ---- CTC phrase search (no reference counterpart): where in each clip is each of K phrases spoken?  The same trellis as
 * dsmi_align with a free start and a free end, over the probabilities dsmi_forward wrote; every phrase is searched in every
 * clip.  The decoder's language model plays no part.
 * probs_dev [B][T_out][n_labels]; sizes_host[B] frames per clip (NULL = T_out for all); phrases_host [K][L_stride] label ids,
 * phrase k's first phrase_lens_host[k] valid, 1 <= length <= L_stride <= DSMI_SPOT_MAX_TOKENS, never the blank.
 * The recurrence (the contract).  A phrase t_1..t_L has S = 2L - 1 states with no leading and no trailing blank: state 2j is
 * token j+1, state 2j+1 the blank between two tokens.  lp(f, c) = logf(fmaxf(p(f, c), FLT_MIN)), accumulated in float32 over
 * frames in order, as dsmi_align does.  Each state carries a score a_f(s) and the frame b_f(s) at which its path began;
 * a_{-1}(s) = -inf, b_{-1}(s) = -1.  For frames f = 0 .. sizes[b]-1:
 *     state 0:  a_f(0) = lp(f, t_1), b_f(0) = f.  (A fresh start scores 0 before the frame's lp and every carried score is
 *               <= 0, so state 0 always restarts: on a tie the later start wins.)
 *     s >= 1:   the predecessor is the best of a_{f-1}(s) and a_{f-1}(s-1) and, for an even s >= 2 with
 *               label(s) != label(s-2), a_{f-1}(s-2); ties as dsmi_align: s before s-1 before s-2, strict > to move.
 *               a_f(s) = best + lp(f, label(s)), b_f(s) = the chosen predecessor's b; a -inf best stays -inf with b = -1.
 * Tracks: E[f] = a_f(S-1), the log probability of the best path that emits exactly the phrase and ends in its last token at
 * frame f, and ST[f] = b_f(S-1), where that path began.
 * Picking, per (clip, phrase).  Candidates: every f with E[f] > -inf and E[f] >= min_mean_logp * (float)(f - ST[f] + 1) (a
 * float32 multiply, no division; min_mean_logp = -inf admits every finite frame).  Up to max_hits times: take the candidate
 * with the largest E (on a tie the lowest f), emit the hit [ST[e], e+1) with score E[e], and drop every candidate f whose
 * [ST[f], f] intersects [ST[e], e]; stop when none is left.  Hits come out best first and are pairwise disjoint.
 * The raw-score optimum is tight: every frame costs, so the first and the last token occupy ONE frame each in the reported
 * span -- a hit starts inside the first character's run and ends inside the last character's run; it is not their extent.
 * Outputs: hits_host [B][K][max_hits][2] frames [start, end); scores_host [B][K][max_hits]; counts_host [B][K]; rows past
 * the count are 0.  track_scores_host / track_starts_host [B][K][T_out] are optional (each is copied back only when
 * not NULL): the E / ST tracks, -inf / -1 at the frames past sizes[b].  A clip with fewer frames than a phrase needs (0
 * frames included) gives count 0.
 * Refused before any launch with nothing written: DSMI_ERR_INVALID for B, T_out or K <= 0, sizes[b] outside 0 .. T_out, a
 * length outside 1 .. L_stride, a token that is the blank or not a label, max_hits outside 1 .. DSMI_SPOT_MAX_HITS, a NaN
 * min_mean_logp; DSMI_ERR_CAPACITY for L_stride > DSMI_SPOT_MAX_TOKENS, K > DSMI_SPOT_MAX_PHRASES, B * K * T_out > 2^27 (the
 * track workspace, kept on the handle).  Two kernel launches whatever B and K.  Synchronises `stream`.
 *
 * dsmi_spot_plan (host only) is the packing dsmi_spot uses: the phrases, in the caller's order, fill groups of at most 256
 * states (one workgroup per group and clip); a phrase that does not fit opens the next group.  group_of[k] / first_state[k]
 * = the group of phrase k and the index of its state 0 in it.  Returns the number of groups; < 0 for NULL arguments, K outside
 * 1 .. DSMI_SPOT_MAX_PHRASES or a length outside 1 .. DSMI_SPOT_MAX_TOKENS. */
#define DSMI_SPOT_MAX_TOKENS 128
#define DSMI_SPOT_MAX_PHRASES 4096
#define DSMI_SPOT_MAX_HITS 64
int dsmi_spot_plan(const int32_t* phrase_lens, int K, int32_t* group_of, int32_t* first_state);
int dsmi_spot(dsmi_decoder* d, const float* probs_dev, const int32_t* sizes_host, int B, int T_out,
              const int32_t* phrases_host, const int32_t* phrase_lens_host, int K, int L_stride,
              int max_hits, float min_mean_logp,
              int32_t* hits_host, float* scores_host, int32_t* counts_host,
              float* track_scores_host, int32_t* track_starts_host, void* stream);

/* ---- Streaming phrase watch (no reference counterpart): dsmi_spot's search carried from one chunk of a live session's
 * probabilities to the next, so that a streaming caller pays for each frame once and hears of a phrase settle_frames frames
 * after it was said.  The recurrence needs one score and one start frame per state from the frame before, nothing else.
 * A dsmi_spot_watch is a phrase list bound to one dsmi_decoder: K phrases as label ids with dsmi_spot's limits (1 <= length <=
 * L_stride <= DSMI_SPOT_MAX_TOKENS, K <= DSMI_SPOT_MAX_PHRASES, never the blank), packed once into dsmi_spot_plan's groups and
 * uploaded once, with the two picking parameters min_mean_logp (as dsmi_spot's; not NaN) and settle_frames >= 1.
 * dsmi_spot_watch_info tells K, the number of groups and settle_frames (each pointer may be NULL).
 * A dsmi_spot_stream is one live utterance's carried search over one watch: a device block of its own with, per state of every
 * group, the float32 score and the int32 start frame of the last frame processed and, per phrase, the picker's state below.
 * dsmi_spot_stream_reset starts a new utterance; dsmi_spot_stream_frames tells the frames consumed since.  A watch serves any
 * number of streams; destroy every stream of a watch before the watch, and every watch before its decoder.
 *
 * dsmi_spot_stream_advance_many advances n distinct streams of one watch in ONE launch whatever n and K (1 <= n <=
 * DSMI_SPOT_STREAM_MANY_MAX): stream i by frames[i] >= 0 rows of probs_dev[i] (device, [frames[i]][n_labels] float32, the
 * softmax output; may be NULL when frames[i] = 0).  flush[i] != 0: the utterance ends with this chunk (a flush with 0 frames is
 * legal).  Frames are counted from the utterance's first frame: this call's frame f of stream i is frame t0 + f, t0 = the
 * frames consumed before.  A call that would take a stream past 2^31 - 1 frames is refused.
 * Tracks (the contract).  E and ST of stream i over all its chunks laid end to end are exactly dsmi_spot's E / ST tracks of the
 * concatenated probabilities -- the same recurrence, tie rule and float32 accumulation in frame order, so they are equal bit
 * for bit however the utterance was cut.  track_scores_host / track_starts_host [n][K][F_stride] are optional (each is copied
 * back only when not NULL; with either, F_stride >= every frames[i]): this call's frames, -inf / -1 past frames[i].
 * The online picking rule (the contract).  Per (stream, phrase): a pending candidate (pv, ps, pe) or none, and last_end
 * (-1 at the utterance's start).  For each frame f in order:
 *   1. a pending candidate with f - pe >= settle_frames fires: the event [ps, pe + 1) with score pv and fired = f;
 *      last_end = pe, and nothing is pending.
 *   2. f is a candidate iff E[f] > -inf, E[f] >= min_mean_logp * (float)(f - ST[f] + 1) (dsmi_spot's float32 multiply) and
 *      ST[f] > last_end.
 *   3. with none pending the candidate becomes pending, (pv, ps, pe) = (E[f], ST[f], f); with one pending and ST[f] <= pe
 *      (the windows meet) it replaces the pending one only if E[f] > pv (strict: the earlier one wins a tie); with one
 *      pending and ST[f] > pe the pending one fires (fired = f, last_end = pe) and f becomes pending.
 * After the last frame of a flushed call the pending candidate fires with fired = the utterance's frame count.  The events of a
 * (stream, phrase) are pairwise disjoint and come out in time order, at most one per frame and phrase.  The rule is a
 * function of the tracks alone: it does not depend on how the utterance was cut into calls.
 * Outputs: hits_host [n][K][max_events][2] frames [start, end), scores_host and fired_host [n][K][max_events], counts_host
 * [n][K] = the events fired in this call; the first min(count, max_events) are stored in firing order and rows past that are
 * 0.  count > max_events: the later ones were dropped -- the stream's state advances all the same.  1 <= max_events <=
 * DSMI_SPOT_MAX_HITS.
 * Either every stream advances or the call is refused before any launch, with no stream's state changed and nothing written;
 * the error text (dsmi_spot_stream_last_error(NULL)) names the stream index.  DSMI_ERR_INVALID: NULL arguments or handles, n
 * outside its range, a handle listed twice, streams of different watches, frames[i] < 0, probabilities missing for frames[i] >
 * 0, max_events outside its range, F_stride below a frames[i] when tracks are asked for.  DSMI_ERR_CAPACITY: n * K * max_events
 * > 2^24 (the events), n * K * F_stride > 2^27 (the tracks), a stream past 2^31 - 1 frames.  Synchronises `stream`.
 *
 * dsmi_spot_watch_pick (host only, no GPU) is the rule itself over caller-supplied tracks of ONE phrase, chunk by chunk:
 * E / ST [frames] are the frames t0 .. t0 + frames - 1, *state is carried from call to call ({0, 0, 0, -1, 0} starts an
 * utterance), flush != 0 ends it.  hits [max_events][2], scores and fired [max_events] take the first min(count, max_events)
 * events (nothing past them is written); returns the count, or DSMI_ERR_INVALID for a NULL state, frames < 0, t0 < 0, t0 +
 * frames > 2^31 - 1, arrays missing for frames > 0, max_events < 0 or outputs missing for max_events > 0, settle_frames < 1,
 * a NaN min_mean_logp.  The kernel runs the same inline function. */
typedef struct dsmi_spot_watch dsmi_spot_watch;
typedef struct dsmi_spot_stream dsmi_spot_stream;
typedef struct {
    int32_t pending;
    int32_t ps;
    int32_t pe;
    int32_t last_end;
    float pv;
} dsmi_spot_pick_state;
#define DSMI_SPOT_STREAM_MANY_MAX 4096
int dsmi_spot_watch_create(dsmi_decoder* d, const int32_t* phrases_host, const int32_t* phrase_lens_host, int K, int L_stride,
                           float min_mean_logp, int settle_frames, dsmi_spot_watch** out);
void dsmi_spot_watch_destroy(dsmi_spot_watch* w);
const char* dsmi_spot_watch_last_error(const dsmi_spot_watch* w);
int dsmi_spot_watch_info(const dsmi_spot_watch* w, int* K, int* n_groups, int* settle_frames);
int dsmi_spot_stream_create(dsmi_spot_watch* w, dsmi_spot_stream** out);
void dsmi_spot_stream_destroy(dsmi_spot_stream* s);
const char* dsmi_spot_stream_last_error(const dsmi_spot_stream* s);
int dsmi_spot_stream_reset(dsmi_spot_stream* s);
int dsmi_spot_stream_frames(const dsmi_spot_stream* s, int64_t* frames);
int dsmi_spot_stream_advance_many(dsmi_spot_stream* const* streams, int n, const float* const* probs_dev, const int32_t* frames,
                                  const int32_t* flush, int max_events, int32_t* hits_host, float* scores_host,
                                  int32_t* fired_host, int32_t* counts_host, float* track_scores_host,
                                  int32_t* track_starts_host, int F_stride, void* stream);
int dsmi_spot_watch_pick(const float* E, const int32_t* ST, int frames, int t0, int flush, float min_mean_logp,
                         int settle_frames, dsmi_spot_pick_state* state, int max_events, int32_t* hits, float* scores,
                         int32_t* fired);

/* ---- CTC transcript scoring (no reference counterpart): how probable is this transcript, summed over every alignment?  The
 * natural log of the probability that the CTC model emits exactly a candidate's label sequence, through the probabilities
 * dsmi_forward wrote.  Every frame's softmax sums to 1, so the likelihoods of all label sequences sum to 1 and exp(logp) is the
 * acoustic model's posterior of the transcript.  The decoder's language model plays no part.
 * probs_dev [B][T_out][n_labels]; sizes_host[B] frames per clip (NULL = T_out for all), as for dsmi_align.  N candidates over
 * the B clips: candidate n belongs to clip cand_clip_host[n] (any order; a clip may have none or many) and its tokens are
 * targets_host[n][0 .. target_lens_host[n]) of targets_host [N][L_stride] (never the blank; 0 tokens is legal).
 * The recurrence (the contract).  The states are dsmi_align's: S = 2L + 1 (blank, t_1, blank, t_2, ..., blank), the same skip
 * rule and the same alpha_0.  Everything is in float64, with lp(t, c) = log((double)fmaxf(p, FLT_MIN)):
 *     alpha_0    = {lp(0, blank), lp(0, t_1), -inf, ...}
 *     alpha_t(s) = logsumexp(alpha_{t-1}(s), alpha_{t-1}(s-1), alpha_{t-1}(s-2) [only if s is a token state and
 *                  label(s) != label(s-2)]) + lp(t, label(s))
 *     logp       = logsumexp(alpha_{T-1}(S-1), alpha_{T-1}(S-2))
 * A log-sum-exp whose arguments are all -inf is -inf, never NaN.  The result is specified as a value with a bound, not bit for
 * bit: |logp - the recurrence evaluated exactly| <= 8 * T * 2^-52 * max(1, |logp|) (log-sum-exp is non-expansive, so the
 * rounding errors of the frames add linearly, a few ulp of |alpha| per frame); how the log-sum-exp is formed is the
 * library's choice.  Frames past sizes[b] are never read.  The scoring is deterministic and batch-invariant: a candidate's
 * result is bit-identical whatever else is in the call.
 * Outputs: logp_host [N] (natural log); status_host [N] = 0 scored, 1 infeasible (the rule of dsmi_align:
 * L + #{k : t_k == t_{k+1}} > frames; then logp = -inf).  0 frames with 0 tokens gives logp = 0.
 * Refused before any launch with nothing written: DSMI_ERR_INVALID for B, T_out or N <= 0, sizes[b] outside 0 .. T_out,
 * cand_clip[n] outside 0 .. B-1, a length outside 0 .. L_stride, a token that is the blank or >= n_labels, NULL outputs;
 * DSMI_ERR_CAPACITY for L_stride > DSMI_SCORE_MAX_TOKENS (LDS: two alpha rows of S doubles per candidate) or
 * N * L_stride > 2^24 (the upload buffer, kept on the handle).  One kernel launch whatever N.  Synchronises `stream`.
 *
 * dsmi_score_plan (host only) is the launch order dsmi_score uses, one workgroup per candidate: order[i] is the candidate
 * workgroup i scores, sorted by cand_frames (the frames of the candidate's clip) descending, so that the longest chains start
 * first; then by clip ascending, so that the candidates of one clip run side by side and share the clip's probabilities in L2;
 * then by token count descending; then by index ascending.  Returns N; < 0 for NULL arguments, N <= 0 or a negative entry. */
#define DSMI_SCORE_MAX_TOKENS 2048
int dsmi_score_plan(const int32_t* cand_clip, const int32_t* cand_frames, const int32_t* target_lens, int N, int32_t* order);
int dsmi_score(dsmi_decoder* d, const float* probs_dev, const int32_t* sizes_host, int B, int T_out,
               const int32_t* cand_clip_host, const int32_t* targets_host, const int32_t* target_lens_host, int N, int L_stride,
               double* logp_host, int32_t* status_host, void* stream);

/* ---- CTC token confidence (no reference counterpart): how sure is the model of THIS token, and what was the runner-up?  For
 * every token of a candidate transcript, the likelihood of the transcript with that token replaced by each other label, or
 * deleted -- all of them from one forward-backward pass, where dsmi_score would need one candidate per edit.
 * probs_dev, sizes_host, cand_clip_host, targets_host, target_lens_host, N and L_stride are dsmi_score's.  Candidate n is a
 * transcript y of L tokens on clip b with T frames.  It has L slots; slot k and label c define a variant transcript:
 *     c != blank:  y with token k replaced by c (c = y_k: y itself);
 *     c  = blank:  y with token k deleted.
 * alt_logp[n][k][c] is the natural log of the probability that the model emits exactly the variant: what dsmi_score's
 * recurrence defines for it (float64, lp = log((double)fmaxf(p, FLT_MIN)), the same states, skip rule and end rule), and -inf
 * where the variant cannot fit the frames (dsmi_align's feasibility rule applied to the variant).  logp[n] is the same for y.
 * exp(alt_logp[n][k][c] - logsumexp_c' alt_logp[n][k][c']) is the posterior of label c in slot k given the rest of y, the
 * blank column being "no token here".  Insertions (a token y lacks) are not covered.
 * The result is specified as a value with a bound, not bit for bit: |value - the recurrence evaluated exactly on the variant|
 * <= 24 * T * 2^-52 * max(1, |value|), three times dsmi_score's, because a result passes through at most three chained float64
 * recurrences of T steps (the forward pass, the backward pass, the slot's own chain), each non-expansive.  It is deterministic
 * and batch-invariant: a candidate's logp and alt_logp rows are bit-identical whatever else is in the call.  Frames past
 * sizes[b] are never read.
 * Outputs: logp_host [N]; alt_logp_host [N][L_stride][n_labels], rows k >= target_lens[n] are -inf; status_host [N] = 0
 * scored, 1 infeasible (then logp = -inf, every alt_logp row -inf, and nothing is computed for the candidate).  0 tokens is
 * legal (no slots, logp as dsmi_score); with 0 frames the empty transcript has logp = 0 and every other candidate is infeasible.
 * Refused before any launch with nothing written: DSMI_ERR_INVALID for everything dsmi_score refuses (alt_logp_host may be NULL
 * only when L_stride == 0); DSMI_ERR_CAPACITY for L_stride > DSMI_ALT_MAX_TOKENS, N * L_stride * n_labels > 2^24 (the
 * results), or a stored trellis -- the sum over the feasible candidates of frames * (2 * length + 1) -- above 2^25 elements
 * (the workspace holds two and a half of them in float64, kept on the handle).  Two kernel launches whatever N.
 * Synchronises `stream`. */
#define DSMI_ALT_MAX_TOKENS 1024
int dsmi_alternatives(dsmi_decoder* d, const float* probs_dev, const int32_t* sizes_host, int B, int T_out,
                      const int32_t* cand_clip_host, const int32_t* targets_host, const int32_t* target_lens_host,
                      int N, int L_stride, double* logp_host, double* alt_logp_host, int32_t* status_host, void* stream);

/* ---- CTC occupancy (no reference counterpart): which frames does each token of a known transcript occupy, and how probable is
 * each label at each frame GIVEN the transcript?  The per-frame posteriors under alignment, scoring and token confidence: soft
 * timings (a token's expected time, dwell and spread over every alignment, not one hard path), and the gradient of the CTC loss.
 * probs_dev, sizes_host, cand_clip_host, targets_host, target_lens_host, N and L_stride are dsmi_score's.  Candidate n is a
 * transcript y of L tokens on clip b with T frames.
 * Definitions (the contract).  The states, the skip rule, alpha_0, lp(t, c) = log((double)fmaxf(p, FLT_MIN)) and logp are
 * dsmi_score's.  beta_t(s) is dsmi_alternatives': the log probability of finishing from state s at frame t, frame t's emission
 * included; at T-1 only S-1 and S-2 are finite:
 *     beta_{T-1}(s) = lp(T-1, label(s)) for s >= S-2, else -inf
 *     beta_t(s)     = logsumexp(beta_{t+1}(s), beta_{t+1}(s+1), beta_{t+1}(s+2) [only if s+2 is a token state and
 *                     label(s+2) != label(s)]) + lp(t, label(s))
 *     gamma_t(s)    = exp(alpha_t(s) + beta_t(s) - lp(t, label(s)) - logp), 0 where alpha or beta is -inf, never NaN
 *     tok[n][t][k]  = gamma_t(2k+1)
 *     occ[n][t][c]  = the sum of gamma_t(s) over the states s with label(s) == c (the blank's column collects the L+1 blank states)
 * Every alignment passes through exactly one state per frame, so each row of occ sums to 1, and
 * d logp / d lp(t, c) = occ[t][c]: the gradient of -logp with respect to the pre-softmax activations is p_t(c) - occ_t(c).
 * Outputs: logp_host [N] and status_host [N] as dsmi_score's (1 = infeasible, logp = -inf).  occ_dev [N][T_out][n_labels] and
 * tok_dev [N][T_out][L_stride] are float64, caller-allocated and stay on the DEVICE: they are as large as the probabilities
 * and their consumers (the gradient, reductions over frames) are there.  Either may be NULL and is then not computed (with
 * L_stride == 0 tok_dev has no element and is ignored).  Both are written in full: rows t >= frames, columns k >= length and
 * everything of an infeasible candidate are 0.0, so the caller never clears them.  With 0 tokens occ_t(blank) is 1 within the
 * bound for t < frames; with 0 frames the empty transcript has logp = 0 and all zeros, every other candidate is infeasible.
 * The results are specified as values with a bound, not bit for bit: logp holds dsmi_score's bound, and every occ and tok
 * element is within 32 * T * 2^-52 * max(1, |logp| + 88) of the recurrences evaluated exactly, in absolute terms.  alpha, beta
 * and logp each carry 8 T 2^-52 max(1, |value|) (each is one non-expansive float64 recurrence of T steps).  For a state with
 * exponent x = alpha + beta - lp - logp <= 0, |alpha| + |beta| <= |x| + |logp| + |lp| with |lp| <= 87.4 (-log FLT_MIN), so the
 * exponent's error is at most 8 T 2^-52 (|x| + 2 |logp| + 91) and that of e^x is e^x times it.  e^x |x| <= 1/e for one state;
 * over the states of one label, with g = e^x and sum g <= 1, sum g |x| <= ln S + 1 < 10 (S <= 2049).  Together at most
 * 8 T 2^-52 (2 |logp| + 101), inside the stated bound; the sum of at most L + 1 <= T + 1 terms itself adds (L + 1) 2^-53.
 * Deterministic and batch-invariant: a candidate's logp, occ and tok are bit-identical whatever else is in the call and from
 * run to run -- a label's sum is formed over the candidate's own tokens in the order of k by one thread, with no floating-point
 * atomic.  Frames past sizes[b] are never read.
 * Refused before any launch with nothing written on host or device: DSMI_ERR_INVALID for everything dsmi_score refuses and for
 * NULL logp_host or status_host; DSMI_ERR_CAPACITY, the limit named in the message, for L_stride > DSMI_OCC_MAX_TOKENS,
 * N * L_stride > 2^24 (the upload buffer, kept on the handle), or a stored trellis -- the sum over the feasible candidates of
 * frames * (2 * length + 1) -- above 2^25 elements (two of them in float64, kept on the handle).  What the numbers alone refuse
 * is refused before any caller array is read.  Two kernel launches whatever N (one when both device arrays are NULL).
 * Synchronises `stream`. */
#define DSMI_OCC_MAX_TOKENS 1024
int dsmi_occupancy(dsmi_decoder* d, const float* probs_dev, const int32_t* sizes_host, int B, int T_out,
                   const int32_t* cand_clip_host, const int32_t* targets_host, const int32_t* target_lens_host,
                   int N, int L_stride, double* logp_host, double* occ_dev, double* tok_dev, int32_t* status_host, void* stream);

/* ---- CTC grammar decoding (no reference counterpart): the text is known only up to a grammar -- commands, digits, a closed
 * vocabulary said any number of times, a transcript with alternatives and optional words.  The most probable frame-level CTC
 * path of ANY sentence a token graph accepts, through the probabilities dsmi_forward wrote: dsmi_align's max-plus recurrence
 * over a graph of token nodes where dsmi_align has a chain.  The decoder's language model plays no part.
 * The graph (the contract).  N nodes; node n has a label lab[n], never the blank; a weight w[n], a finite float32 added once
 * when the node is entered; a start flag and a final flag; an ordered list of predecessor nodes pred[n][0..), stored as CSR.
 * Cycles and self-loops are legal (a self-loop is "the same token again", which CTC lets through only over a blank).  empty_ok:
 * the empty sentence is accepted.  Each node carries two states, tok(n) and blk(n) (the blank after it); one more state, lead,
 * is the blank before the first token.  With lp(t, c) = logf(fmaxf(p, FLT_MIN)), everything float32 and accumulated in frame
 * order:
 *     t = 0:  lead = lp(0, blank);  tok(n) = start[n] ? lp(0, lab[n]) + w[n] : -inf;  blk(n) = -inf
 *     t >= 1: ent(n)  = max{ lead [if start[n]];  for j in order: blk(pred j), then tok(pred j) [only if lab[pred j] != lab[n]] }
 *             tok'(n) = max(tok(n), ent(n) + w[n]) + lp(t, lab[n])
 *             blk'(n) = max(blk(n), tok(n)) + lp(t, blank)
 *             lead'   = lead + lp(t, blank)
 *     end:    max{ lead [if empty_ok];  for final n ascending: blk(n), then tok(n) }
 * Tie rule (part of the contract): a later candidate replaces an earlier one only when strictly greater, the candidates taken
 * in the order written: stay before any entry; among entries lead, then the predecessors in list order, each blk before tok;
 * entries are compared before w[n] is added; for blk', stay before tok.  With this order a chain graph (node k's only
 * predecessor is k-1, node 0 start, node L-1 final, empty_ok = (L == 0), weights 0) gives dsmi_align's results bit for bit.
 * Inputs: probs_dev [B][T_out][n_labels]; sizes_host [B] frames per clip (NULL = T_out for all).  pool: K graphs concatenated.
 * Graph g owns the nodes node_off[g] .. node_off[g+1] of labels, weights (NULL = all 0) and flags (DSMI_GRAMMAR_START |
 * DSMI_GRAMMAR_FINAL); node i of the pool has the predecessors arc_pred[arc_off[i] .. arc_off[i+1]), graph-local ids; node_off
 * [K+1] and arc_off [node_off[K] + 1] ascend from 0; empty_ok [K] (non-zero = accepted).  clip_graph_host [B] = the graph of
 * each clip (NULL = graph 0 for all): one grammar for many clips, or each clip its own transcript graph.  A graph without
 * nodes is legal and accepts exactly the empty sentence, when empty_ok holds.
 * Outputs per clip, host arrays, the three path arrays with row stride T_out (a path has at most one visit per frame):
 * path_lens [B] = M, the node visits (a visit: a maximal run of consecutive frames in tok(n) linked by "stay"); path_nodes
 * [B][T_out] graph-local node ids; path_spans [B][T_out][2] frames [start, end); token_probs [B][T_out] = the float32 mean
 * of p(t, lab) over the span, summed in frame order; path_logp [B], weights included; status [B] = 0 decoded, 1 when no
 * accepted sentence fits the clip's frames (path_logp = -inf, M = 0).  Rows past M are 0.  lp >= logf(FLT_MIN) is finite, so
 * -inf at the end means unreachable and nothing else: the device decides the status.  A clip of 0 frames is decoded only
 * when empty_ok holds (path_logp = 0).  A clip's results are the same bits whatever else is in the call.
 * Refused before any launch with nothing written (DSMI_ERR_INVALID, each fault with its own message): B, T_out or K <= 0, a
 * NULL argument (weights and clip_graph_host may be NULL), sizes[b] outside 0 .. T_out, clip_graph[b] outside 0 .. K-1,
 * offsets that do not start at 0 or do not ascend, a label that is the blank or >= n_labels, a predecessor outside its graph,
 * a weight that is NaN or infinite, a graph with nodes but no start node or no final node.  DSMI_ERR_CAPACITY, the limit
 * named: a graph of more than DSMI_GRAMMAR_MAX_NODES nodes or DSMI_GRAMMAR_MAX_ARCS arcs (LDS: two double-buffered float32
 * rows per node, the node words, weights and offsets, the arcs as 16-bit words, the probabilities' image: 84 KB of 160 KB at
 * both limits), more than 2^24 nodes or arcs in the pool, more than 2^31 bytes of backpointers (2 * B * T_out * node stride,
 * kept on the handle; 66 MB for 32 clips of 501 frames at the node limit).  What the numbers alone refuse (B, T_out, K) is
 * refused before any array is read.  One kernel launch, one workgroup per clip.  Synchronises `stream`.
 * dsmi_grammar_plan (host only, no handle): for a call of B clips of T_out frames whose largest graph has n_nodes nodes and
 * n_arcs arcs, info = {node stride (n_nodes rounded up to a multiple of 4, at least 4), LDS bytes per workgroup, backpointer
 * workspace bytes}.  Returns DSMI_OK, or the code with which dsmi_grammar would refuse these numbers; DSMI_ERR_INVALID for a
 * NULL info. */
#define DSMI_GRAMMAR_MAX_NODES 2048
#define DSMI_GRAMMAR_MAX_ARCS 8192
#define DSMI_GRAMMAR_START 1
#define DSMI_GRAMMAR_FINAL 2
typedef struct {
    int32_t K;                   /* graphs */
    const int32_t* node_off;     /* [K + 1] */
    const int32_t* labels;       /* [node_off[K]] */
    const float* weights;        /* [node_off[K]], or NULL = 0 */
    const int32_t* flags;        /* [node_off[K]] DSMI_GRAMMAR_START | DSMI_GRAMMAR_FINAL */
    const int32_t* arc_off;      /* [node_off[K] + 1] */
    const int32_t* arc_pred;     /* [arc_off[node_off[K]]] graph-local node ids */
    const int32_t* empty_ok;     /* [K] */
} dsmi_grammar_pool;
int dsmi_grammar(dsmi_decoder* d, const float* probs_dev, const int32_t* sizes_host, int B, int T_out,
                 const dsmi_grammar_pool* pool, const int32_t* clip_graph_host, int32_t* path_lens_host,
                 int32_t* path_nodes_host, int32_t* path_spans_host, float* token_probs_host, float* path_logp_host,
                 int32_t* status_host, void* stream);
int dsmi_grammar_plan(int B, int T_out, int n_nodes, int n_arcs, int64_t* info);

/* ---- CTC grammar posterior (no reference counterpart): was a sentence of the grammar said at all, how sure is the decoded
 * sentence given that one was, which label does each frame carry given the grammar, and how much probability flows through each
 * node?  dsmi_grammar's recurrence in the log-sum-exp semiring: the all-paths half of the word-graph tools, as dsmi_score and
 * dsmi_occupancy are of the transcript tools.  A CTC model's frame rows each sum to 1, so the probabilities of all labellings
 * sum to 1 and the summed probability of every path the graph accepts is a posterior that needs no garbage model.
 * probs_dev, sizes_host, pool and clip_graph_host are dsmi_grammar's, and so are the states: lead, tok(n) and blk(n).
 * Everything is float64, with lp(t, c) = log((double)fmaxf(p, FLT_MIN)) as in dsmi_score and the float32 weights widened; a
 * weight is added once, on entry to its node.  LSE is log-sum-exp; one whose arguments are all -inf is -inf, never NaN.
 *     t = 0:  lead = lp(0, blank);  tok(n) = start[n] ? lp(0, lab[n]) + w[n] : -inf;  blk(n) = -inf
 *     t >= 1: ent(n)  = LSE{ lead [if start[n]];  per predecessor p: blk(p), and tok(p) only if lab[p] != lab[n] }
 *             tok'(n) = LSE(tok(n), ent(n) + w[n]) + lp(t, lab[n])
 *             blk'(n) = LSE(blk(n), tok(n)) + lp(t, blank)
 *             lead'   = lead + lp(t, blank)
 *     end:    logp = LSE{ lead [if empty_ok];  per final n: blk(n), tok(n) }
 * These are alpha_t.  beta_t(state) is the mirror image over the successor lists: the log of the summed probability of every
 * way to finish from the state at frame t, frame t's emission and the weights of the nodes still to be entered included; at the
 * last frame beta = lp(T-1, label) for tok and blk of a final node and for lead when empty_ok holds, else -inf.
 *     gamma_t(state) = exp(alpha_t + beta_t - lp(t, label(state)) - logp), 0 where alpha or beta is -inf, never NaN
 *     occ[b][t][c]   = the sum of gamma_t over the states carrying label c (the blank's column collects lead and every blk)
 *     visits[b][n]   = the sum over t of the posterior of ENTERING tok(n) at frame t: gamma_t(tok n) less the share that was in
 *                      tok(n) at t-1 already; a start node's occupancy at frame 0 counts as an entry
 * Every path is in exactly one state per frame, so each row of occ with t < frames sums to 1, and d logp / d lp(t, c) =
 * occ[t][c]: the gradient of the graph loss, as dsmi_occupancy's occ is of the transcript loss.  visits[n] = d logp / d w[n], the
 * expected number of entries into node n: at most 1 on an acyclic graph, and on a hand-built graph with one node per slot value
 * the slot's posterior.
 * Paths, not sentences.  The sum runs over the paths of the graph -- sequences of states -- and not over sentences: a sentence
 * that two node sequences spell counts twice, and a predecessor listed twice is two arcs.  exp(logp) is the probability of the
 * grammar's language exactly when the graph is unambiguous (no sentence has two node sequences) and its weights are 0; then
 * exp(dsmi_score's logp of a sentence - logp) is the sentence's posterior given that a sentence of the grammar was said.
 * Outputs: logp_host [B] float64; status_host [B] = 0 decoded, 1 when no accepted sentence fits the clip's frames (logp = -inf);
 * lp is finite, so -inf at the end means unreachable and nothing else: the device decides the status.  visits_host
 * [B][N_stride] float64, may be NULL; N_stride >= the most nodes of any graph of the pool, columns past a graph's nodes are 0.
 * occ_dev [B][T_out][n_labels] float64, caller-allocated, stays on the DEVICE, may be NULL.  Everything is written in full: rows
 * t >= sizes[b] are 0.0 and an infeasible clip is all zeros, so the caller never clears them.  A clip of 0 frames is decoded
 * only when empty_ok holds (logp = 0, all zeros).
 * The results are values with a bound, not fixed bits.  With F the largest number of predecessors of one node in the call's
 * graphs and k(F) = 32 + (F + 1) / 8: logp is within 8 * T * 2^-52 * max(1, |logp|) + (F + 1) * T * 2^-52 of the recurrence
 * evaluated exactly (dsmi_score's form and the term below), every occ element within
 *     bound = k(F) * T * 2^-52 * max(1, |logp| + 88)
 * in absolute terms, and every visits element within T * bound.  The derivation is dsmi_occupancy's with one added term.  One
 * step is a log-sum-exp of up to 2F + 1 terms where a transcript's has 3: formed as the greatest term m, the sum of exp(x - m)
 * and one log, the sum of at most 2F + 1 terms in [0, 1] with one of them 1 carries a relative error of at most (2F + 1) 2^-53,
 * which the log turns into as much absolute error of the step, on top of the few ulp of |alpha| per frame that make up the
 * 8 T 2^-52 max(1, |value|) of alpha, beta and logp each.  The exponent of gamma has three such values, so the added term is
 * 3 (2F + 1) T 2^-53 <= ((F + 1) / 8) T 2^-52 * 88, and e^x <= 1 passes it on as it stands; the rest -- |alpha| + |beta| <= |x| +
 * |logp| + |lp|, sum g |x| <= ln(states) + 1 over the at most 4097 states of one label -- is dsmi_occupancy's and stays inside
 * 32.  (It takes alpha and beta to be <= 0: weights that are log probabilities.  Positive weights add the greatest sum of them
 * along one path to |logp| in the bound.)  visits is a sum over T frames of differences of two such terms, each within the
 * bound: T times it, the cancellation being absolute.  The sums of occ (at most 2049 terms of sum <= 1) add 2049 * 2^-53.
 * Deterministic and batch-invariant: a clip's logp, visits and occ are the same bits whatever else is in the call and from run
 * to run.  There is no floating-point atomic, and the order of every sum is fixed by the graph alone: a node's entry over its
 * predecessor list in order, the backward pass over its successors ascending (a node with more than 24 of either: lane l of a
 * wave over the arcs l, l + 64, ... in order, then the lanes in a fixed tree), the end and the start nodes in a fixed tree over
 * ascending nodes, a label's occ over its nodes ascending, a node's visits over the frames in order.  Frames past sizes[b] are
 * never read.
 * Refused before any launch with nothing written on host or device: everything dsmi_grammar refuses, with its codes and
 * messages (the same check); DSMI_ERR_INVALID for a NULL logp_host or status_host, and for N_stride below the pool's largest
 * graph when visits_host is given; DSMI_ERR_CAPACITY, the limit named in the message, when the stored trellises -- B * T_out *
 * (32 * node stride + 16) bytes, two float64 (tok, blk) pairs per frame and node and lead, kept on the handle -- exceed 2^30
 * bytes (32 clips of 501 frames fit at DSMI_GRAMMAR_MAX_NODES: 1002 MiB; a loop over 300 words compiles to about 1000 to 1500 nodes: 510 to 734 MiB).  The
 * graph limits are dsmi_grammar's: at both, a workgroup's LDS holds two double-buffered 16-byte pairs per node (64 KB), node
 * words, weights, offsets and start nodes (24 KB), the arcs (16 KB), the float64 image of the probabilities (32 KB), the end's
 * reduction and the list of wave-reduced nodes (3 KB): 139 KB of 160 KB.  What the numbers alone refuse (B, T_out, and the cap at the least node stride) is refused
 * before any array is read.  Three kernel launches whatever B (one when visits_host and occ_dev are both NULL: the forward pass
 * alone).  Synchronises `stream`.
 * dsmi_grammar_posterior_plan (host only, no handle): for a call of B clips of T_out frames whose largest graph has n_nodes nodes
 * and n_arcs arcs, info = {node stride (n_nodes rounded up to a multiple of 4, at least 4), LDS bytes per workgroup, workspace
 * bytes}.  Returns DSMI_OK, or the code with which dsmi_grammar_posterior would refuse these numbers; DSMI_ERR_INVALID for a NULL
 * info. */
int dsmi_grammar_posterior(dsmi_decoder* d, const float* probs_dev, const int32_t* sizes_host, int B, int T_out,
                           const dsmi_grammar_pool* pool, const int32_t* clip_graph_host, int N_stride,
                           double* logp_host, double* visits_host, double* occ_dev, int32_t* status_host, void* stream);
int dsmi_grammar_posterior_plan(int B, int T_out, int n_nodes, int n_arcs, int64_t* info);

/* ---- Streaming grammar decoding (no reference counterpart): dsmi_grammar's search carried from one chunk of a live session's
 * probabilities to the next, so that a streaming caller pays for each frame once and neither keeps the rows nor packs the
 * graph again.  A dsmi_grammar_net is a pool of K graphs bound to one dsmi_decoder: dsmi_grammar_net_create applies
 * dsmi_grammar's rules to the pool (the same faults, codes and messages; the clip and size rules have nothing to apply to),
 * packs the arcs as dsmi_grammar does, lists the nodes with more than 32 predecessors and uploads once.
 * dsmi_grammar_net_info tells K and the most nodes and arcs of one graph (each pointer may be NULL).  A dsmi_grammar_stream is
 * one live utterance's carried search over graph `graph` of a net, for at most max_frames frames (1 <= max_frames <=
 * DSMI_GRAMMAR_STREAM_MAX_FRAMES): one device block with a 16-byte header (lead and the frame count), the float32 tok / blk
 * pair of every node as of the last frame consumed, the probability rows consumed [max_frames][n_labels] float32 (the
 * per-visit means need them) and the 16-bit backpointers [max_frames][node stride] of the frames consumed.
 * dsmi_grammar_stream_reset starts a new utterance (nothing of the block is read again); dsmi_grammar_stream_frames tells the
 * frames consumed since.  A net serves any number of streams; destroy every stream before its net, and every net before its
 * decoder.
 * dsmi_grammar_stream_plan (host only, no handle): for a graph of n_nodes nodes and n_arcs arcs, n_labels labels and
 * max_frames frames, info = {node stride, LDS bytes per workgroup, device bytes per stream}.  DSMI_ERR_INVALID: a NULL info,
 * max_frames < 1, negative counts, n_labels outside 1 .. 128; DSMI_ERR_CAPACITY: max_frames above
 * DSMI_GRAMMAR_STREAM_MAX_FRAMES, node or arc counts above dsmi_grammar's limits, a block above 2^31 bytes.  (At 1500 frames a
 * 28-node digit loop needs 84 KB of backpointers, the node limit 6.1 MB.)
 *
 * dsmi_grammar_stream_advance_many advances n distinct streams of one net in ONE launch whatever n (1 <= n <=
 * DSMI_GRAMMAR_STREAM_MANY_MAX), one workgroup per stream: stream i by frames[i] >= 0 rows of probs_dev[i] (device,
 * [frames[i]][n_labels] float32, the softmax output; may be NULL when frames[i] = 0).  mode[i] = 0: advance only; 1: advance,
 * then report the partial result; 2: advance, then report the final result -- the utterance is over, and a later call with
 * frames > 0 on this stream is refused until dsmi_grammar_stream_reset.  A call in which no stream has frames or a result due
 * launches nothing.
 * The contract is equality with dsmi_grammar.  Let X be the rows of stream i over all its calls laid end to end and F their
 * count.  With mode 2 the six outputs of stream i -- path_lens, path_nodes, path_spans, token_probs, path_logp, status -- are
 * the bits dsmi_grammar gives for the single clip X (B = 1, T_out = F) on the stream's graph, however the utterance was cut
 * into calls and whatever else is in the call.  With mode 1 they are the bits dsmi_grammar gives for X on the same graph with
 * EVERY node final and empty_ok = 1: the best path into any state, lead first, then the nodes ascending, blk before tok -- the
 * same tie rule -- and complete_host[i] = 1 when that path's end state is one the real graph accepts (lead with the graph's
 * empty_ok, or a node with DSMI_GRAMMAR_FINAL).  With mode 2 complete_host[i] = 1 - status.  With F = 0, mode 2 gives
 * dsmi_grammar's zero-frame result and mode 1 the empty path with path_logp 0, status 0 and complete = empty_ok.
 * Outputs, host arrays: path_lens, path_logp, status and complete [n]; path_nodes and token_probs [n][P_stride], path_spans
 * [n][P_stride][2]; P_stride >= the utterance's frame count after this call of every stream with mode != 0.  Rows past M are
 * 0.  A stream with mode 0 has nothing written for it; complete_host may be NULL.
 * A node with more than 32 predecessors is entered by a whole wave whose lanes stride the list; the reduction takes the
 * greater value and, among equal values, the earlier candidate, which is the sequential rule exactly: no bit depends on it.
 * Either every stream advances or the call is refused before any launch, with no stream's state changed and nothing written;
 * the error text (dsmi_grammar_stream_last_error(NULL)) names the stream index.  DSMI_ERR_INVALID: NULL arguments or handles,
 * n outside its range, a handle listed twice, streams of different nets, frames[i] < 0, probabilities missing for frames[i] >
 * 0, a mode outside 0 .. 2, frames for a stream that has ended, P_stride below the frame count of a stream with mode != 0, a
 * NULL output when any mode != 0.  DSMI_ERR_CAPACITY: a stream that would pass its max_frames (the message says both
 * numbers), n * P_stride > 2^24.  Synchronises `stream`. */
typedef struct dsmi_grammar_net dsmi_grammar_net;
typedef struct dsmi_grammar_stream dsmi_grammar_stream;
#define DSMI_GRAMMAR_STREAM_MANY_MAX 4096
#define DSMI_GRAMMAR_STREAM_MAX_FRAMES (1 << 20)
int dsmi_grammar_net_create(dsmi_decoder* d, const dsmi_grammar_pool* pool, dsmi_grammar_net** out);
void dsmi_grammar_net_destroy(dsmi_grammar_net* n);
const char* dsmi_grammar_net_last_error(const dsmi_grammar_net* n);
int dsmi_grammar_net_info(const dsmi_grammar_net* n, int* K, int* max_nodes, int* max_arcs);
int dsmi_grammar_stream_create(dsmi_grammar_net* n, int graph, int max_frames, dsmi_grammar_stream** out);
void dsmi_grammar_stream_destroy(dsmi_grammar_stream* s);
const char* dsmi_grammar_stream_last_error(const dsmi_grammar_stream* s);
int dsmi_grammar_stream_reset(dsmi_grammar_stream* s);
int dsmi_grammar_stream_frames(const dsmi_grammar_stream* s, int64_t* frames);
int dsmi_grammar_stream_advance_many(dsmi_grammar_stream* const* streams, int n, const float* const* probs_dev,
                                     const int32_t* frames, const int32_t* mode, int P_stride, int32_t* path_lens_host,
                                     int32_t* path_nodes_host, int32_t* path_spans_host, float* token_probs_host,
                                     float* path_logp_host, int32_t* status_host, int32_t* complete_host, void* stream);
int dsmi_grammar_stream_plan(int n_nodes, int n_arcs, int n_labels, int max_frames, int64_t* info);

/* ---- Batched edit distance (the reference calls Levenshtein.distance once per pair, on the host): how far is this text from
 * that one, for many pairs at once -- WER / CER with their error counts, and the pairwise distances of n-best lists.
 * A pool of M token sequences: seqs_host [M][L_stride] with seq_lens_host [M].  Tokens are any int32 and are compared for
 * equality only (word ids or label ids; nothing is special about 0, negative values or the blank).  N pairs index the pool:
 * pair n compares a = sequence pair_a_host[n] (the reference) with b = sequence pair_b_host[n] (the hypothesis).  A sequence
 * may appear in any number of pairs, in either role, or paired with itself.
 * Output: counts_host[n] = {distance, substitutions, deletions, insertions}.  A deletion is a token of a with no partner in b,
 * an insertion a token of b with no partner in a.  The four numbers are those of the minimum-distance alignment with the
 * FEWEST SUBSTITUTIONS: with H matches, H+S+D = La, H+S+I = Lb and S+D+I = d leave one degree of freedom given d, so "fewest
 * substitutions" is also "most matches" and fixes all four uniquely.
 * The recurrence (the contract).  Costs are unsigned 32-bit integers d << 16 | s.  A match adds 0, a substitution SUB = 0x10001,
 * a deletion DEL or an insertion INS 0x10000:
 *     D[i][0] = i << 16,  D[0][j] = j << 16,
 *     D[i][j] = min3(D[i-1][j] + DEL, D[i][j-1] + INS, D[i-1][j-1] + (a_i == b_j ? 0 : SUB))
 * The minimum of packed integers is the lexicographic minimum of (distance, substitutions).  With d, s = D[La][Lb]:
 *     deletions = (d - s - (Lb - La)) / 2,  insertions = deletions + Lb - La.
 * Lengths <= DSMI_EDIT_MAX_TOKENS keep both fields below 2^16.  Results are exact integers: deterministic and batch-invariant.
 * Pairs with an empty side are answered by the host (all deletions or all insertions; 0 for both empty) and nothing is
 * launched for them.  One kernel launch whatever N (none when every pair has an empty side).  Synchronises `stream`.
 * Refused with nothing written and nothing launched: DSMI_ERR_INVALID for M or N <= 0, a length outside 0 .. L_stride, a pair
 * index outside 0 .. M-1, a NULL array (seqs_host may be NULL only when L_stride == 0); DSMI_ERR_CAPACITY for
 * L_stride > DSMI_EDIT_MAX_TOKENS, M * L_stride > 2^24 or N > 2^24 (the upload buffer, kept on the handle).
 *
 * dsmi_edit_plan (host only) is the launch plan dsmi_edit_distance uses for pairs of these lengths.  seg[n] is the lane
 * segment pair n occupies: 16 if len_b <= 16, 32 if len_b <= 32, else 64 (written for every pair).  order[0 .. returned) is
 * the launch order of the pairs that need the kernel (both lengths > 0): by seg ascending; then by work
 * ceil(len_b / 64) * (len_a + seg) descending, so that wave-mates finish together and the longest chains start first; then by
 * index ascending.  A wave takes 64 / seg consecutive pairs of one segment width.  Returns the number of pairs launched;
 * < 0 for NULL arguments, N <= 0 or a negative length. */
#define DSMI_EDIT_MAX_TOKENS 4096
int dsmi_edit_plan(const int32_t* len_a, const int32_t* len_b, int N, int32_t* order, int32_t* seg);
int dsmi_edit_distance(dsmi_decoder* d, const int32_t* seqs_host, const int32_t* seq_lens_host, int M, int L_stride,
                       const int32_t* pair_a_host, const int32_t* pair_b_host, int N, int32_t* counts_host, void* stream);

/* ---- LM sentence scoring: the n-gram score of known sentences with the tables dsmi_decoder_set_lm left on the device -- to
 * rescore an n-best list, to score arbitrary texts, and to tune alpha and beta on the n-best lists of one search.
 * A pool of M label-id sequences: seqs_host [M][L_stride] with seq_lens_host [M], the layout of dsmi_score's candidates and of
 * dsmi_edit_distance's pool; the ids are the decoder's labels.  Nothing past seq_lens_host[m] in a row is read as a token.
 * Words.  A word is a maximal run of tokens other than the space label: leading, trailing and doubled spaces make no empty
 * words.  A decoder whose labels have no space treats every sequence as one word.  A word's id is what the dictionary trie
 * gives for its labels, or -1 (out of vocabulary) if an arc is missing or no word ends at its node; n_oov_host[m] counts the
 * words with id -1, n_words_host[m] all of them.
 * Terms (the contract: ctcdecode Scorer::get_sent_log_prob, window for window).  With s = [<s>] * (order - 1) + words + [</s>],
 * or [<s>] * order + [</s>] for no words, term i is the window s[i .. i + order): -1000 (OOV_SCORE) if any member is out of
 * vocabulary or <unk>, else (double)log10 p(last | the others) / (double)0.4342944819f, the log10 by back-off in float32 as
 * dsmi_lm_cond_log10 gives it.  n_terms_host[m] = n_words + 1, or 2 for no words.  terms_host[m][0 .. n_terms) holds them
 * ([M][W_stride]; entries behind are left alone); terms_host may be NULL, and then W_stride is ignored.  lm_ln_host[m] is their
 * sum in float64, in window order, from 0.0.
 * Every result is exact: the bits dsmi_lm_sentence_ln gives on the host, whatever else is in the call (batch-invariant,
 * deterministic).  One kernel launch whatever M.  Synchronises `stream`.
 * Refused with nothing written and nothing launched: DSMI_ERR_INVALID for a decoder without a language model, M <= 0, a NULL
 * array other than terms_host (seqs_host may be NULL only when L_stride == 0), a length outside 0 .. L_stride, a token outside
 * 0 .. n_labels-1 or equal to the blank; DSMI_ERR_CAPACITY for L_stride > DSMI_LM_SCORE_MAX_TOKENS, M * L_stride > 2^24, or
 * terms_host given with W_stride below the largest n_terms.
 *
 * dsmi_lm_score_plan (host only) is the word segmentation dsmi_lm_score uses, with `space` the space label's id (any value no
 * token has: one word per non-empty row): n_words[m], and the first token and the length of each word in word_first /
 * word_len [M][W_stride].  Returns the largest n_words; < 0 with nothing written for NULL arguments (seqs_host may be NULL
 * only when L_stride == 0, the word arrays only when W_stride == 0), M <= 0, a negative L_stride or W_stride, a length outside
 * 0 .. L_stride, or a row of more than W_stride words.
 *
 * dsmi_lm_sentence_ln (host only, on a dsmi_lm handle) is Scorer::get_sent_log_prob with its terms exposed: the sum for the n
 * words word_ids (the file's own ids; anything outside them, such as -1, is out of vocabulary), and the n + 1 terms (2 for
 * n = 0) in terms[0 .. capacity) unless terms is NULL.  NaN for a NULL handle, n < 0, NULL word_ids with n > 0, or a capacity
 * below the number of terms. */
#define DSMI_LM_SCORE_MAX_TOKENS 4096
typedef struct dsmi_lm dsmi_lm;      /* (the host-only handle: below) */
int dsmi_lm_score_plan(const int32_t* seqs_host, const int32_t* seq_lens_host, int M, int L_stride, int space,
                       int32_t* n_words, int32_t* word_first, int32_t* word_len, int W_stride);
int dsmi_lm_score(dsmi_decoder* d, const int32_t* seqs_host, const int32_t* seq_lens_host, int M, int L_stride,
                  double* lm_ln_host, int32_t* n_words_host, int32_t* n_oov_host,
                  int32_t* n_terms_host, double* terms_host, int W_stride, void* stream);
double dsmi_lm_sentence_ln(const dsmi_lm* lm, const int32_t* word_ids, int n, double* terms, int capacity);

/* ---- Host-only view of a language model file (no GPU involved): what dsmi_decoder_set_lm would load.
 * kind: 0 ARPA text, 1 KenLM probing binary, 2 KenLM trie binary.  Word ids are the file's own (KenLM's WordIndex for
 * binaries, <unk> = 0).  dsmi_lm_lookup: 1 = the n-gram ids[0..n) is in the model (its log10 probability and back-off
 * weight are returned), 0 = absent.  dsmi_lm_cond_log10 = log10 p(ids[n-1] | ids[0..n-1)) by back-off, the quantity the
 * beam search's scorer adds (ctcdecode Scorer::get_log_cond_prob / KenLM BaseScore). */
int dsmi_lm_open(const char* path, dsmi_lm** out);
void dsmi_lm_close(dsmi_lm* lm);
const char* dsmi_lm_last_error(const dsmi_lm* lm);
int dsmi_lm_info(const dsmi_lm* lm, int* order, int64_t* vocab_size, int* kind);
int dsmi_lm_word_index(const dsmi_lm* lm, const char* word_utf8);
int dsmi_lm_lookup(const dsmi_lm* lm, const int32_t* ids, int n, float* log10_prob, float* log10_backoff);
double dsmi_lm_cond_log10(const dsmi_lm* lm, const int32_t* ids, int n);

/* ---- What a handle was built with (a host that received handles from elsewhere, and dsmi_session_create). */
int dsmi_model_info(const dsmi_model* m, dsmi_model_desc* desc, int* device);
int dsmi_frontend_info(const dsmi_frontend* f, int* n_freq, int* hop, int* device);
int dsmi_decoder_info(const dsmi_decoder* d, int* n_labels, int* blank_index, int* device);
const char* dsmi_decoder_label(const dsmi_decoder* d, int index);          /* labels[index] as UTF-8, NULL out of range */

/* ---- Recognizer.recognize (Recognizer.py:158-189) -> DanSpeechRecognizer.transcribe (DanSpeechRecognizer.py:191-231)
 * over a batch of recordings, as ONE call for hosts without the Python layer: stage + upload the clips, spectrograms,
 * network, decoder, label strings, results in the caller's order -- the sequence of dsmi_features, dsmi_forward,
 * dsmi_forward_status, dsmi_greedy / dsmi_beam calls danspeech_amd/DanSpeechRecognizer.py issues.  A session binds one
 * frontend, one model and one decoder of the same device and owns the buffers between the stages and a stream; the
 * handles must outlive it.  One batch per session at a time; a host that keeps two batches in flight uses two sessions
 * (each with its own model and frontend handle, dsmi_model_set_inflight(2) on both) and alternates
 * dsmi_recognize_enqueue / dsmi_recognize_collect between them.
 *   clips_host[b]      clip b's samples in host memory, n_samples_host[b] of them (frames for DSMI_PCM_STEREO), any order
 *   beam_width         0: greedy (a recogniser without language model, DanSpeechRecognizer.py:94); > 0: beam search with
 *                      the decoder's dsmi_decoder_set_lm settings, best beam returned
 *   text_utf8          [B][text_stride]: clip b's transcript, NUL-terminated; one longer than text_stride - 1 bytes is cut
 *                      at a label boundary and text_bytes_host[b] (optional) holds its full length
 *   scores_host        optional [B]: the best beam's score (0 for greedy)
 * Returns DSMI_OK, DSMI_RECOMPUTED (results valid, see dsmi_forward_status) or < 0. */
typedef struct dsmi_session dsmi_session;
int dsmi_session_create(dsmi_frontend* f, dsmi_model* m, dsmi_decoder* d, dsmi_session** out);
void dsmi_session_destroy(dsmi_session* s);
const char* dsmi_session_last_error(const dsmi_session* s);
int dsmi_recognize_batch(dsmi_session* s, const void* const* clips_host, const int64_t* n_samples_host, int pcm_dtype, int B,
                         int beam_width, int cutoff_top_n, double cutoff_prob,
                         char* text_utf8, int text_stride, int32_t* text_bytes_host, float* scores_host);
/* The two halves: everything up to the probabilities, asynchronous; then wait + decode + strings. */
int dsmi_recognize_enqueue(dsmi_session* s, const void* const* clips_host, const int64_t* n_samples_host, int pcm_dtype, int B);
/* Clips already back to back in device memory, LONGEST FIRST (DSMI_ERR_UNSORTED otherwise) -- a shard as
 * dsmi_comm_scatter delivers it: no host staging.  pcm_dev must stay valid until the collect; results are in that order. */
int dsmi_recognize_enqueue_device(dsmi_session* s, const void* pcm_dev, const int64_t* n_samples_host, int pcm_dtype, int B);
int dsmi_recognize_collect(dsmi_session* s, int beam_width, int cutoff_top_n, double cutoff_prob,
                           char* text_utf8, int text_stride, int32_t* text_bytes_host, float* scores_host);

/* ---- Utterance-level data parallelism, one process (or host thread) per GPU, for hosts without torch.distributed
 * (the Python layer: danspeech_amd/parallel.py).  The reference has no distributed code; clips are independent
 * on this path, weights are replicated, and the only exchanges are the input scatter and the result gather: grouped
 * ncclSend / ncclRecv between the root and the other ranks over RCCL, which is bound at run time (dlopen; DSMI_RCCL_LIBRARY
 * overrides the library name) so that libdsmi.so has no load-time dependency on it.
 * dsmi_plan_shards (host only): clips sorted by length, descending and stable, dealt round-robin -- clip i goes to rank
 * rank_of[i] as that rank's slot_of[i]-th clip, so every shard is longest first with a similar length mix.
 * dsmi_comm_unique_id: rank 0 creates the 128-byte id and ships it to the other ranks by the host's own means.
 * dsmi_comm_scatter: the root passes its clips (the other ranks NULL / 0); every rank receives *shard_count clips back to
 * back in device memory at *shard_pcm_dev (library-owned, valid until the next scatter), their lengths and their
 * positions in the root's list (at most shard_cap), the sample type and the batch's total clip count.
 * dsmi_comm_gather_text: every rank passes its shard's transcripts [shard_count][text_stride] with those positions; the
 * root's all_text [total_count][text_stride] receives them in the root's order.  Both synchronise `stream`. */
typedef struct dsmi_comm dsmi_comm;
int dsmi_plan_shards(const int64_t* n_samples, int n, int world, int32_t* rank_of, int32_t* slot_of);
int dsmi_comm_unique_id(void* id128);
int dsmi_comm_init(const void* id128, int rank, int world, int device, dsmi_comm** out);
void dsmi_comm_destroy(dsmi_comm* c);
const char* dsmi_comm_last_error(const dsmi_comm* c);
int dsmi_comm_scatter(dsmi_comm* c, int root, const void* const* clips_host, const int64_t* n_samples_host, int pcm_dtype, int n,
                      const void** shard_pcm_dev, int64_t* shard_n_samples, int32_t* shard_index, int shard_cap,
                      int* shard_count, int* shard_dtype, int* total_count, void* stream);
int dsmi_comm_gather_text(dsmi_comm* c, int root, const char* text, int text_stride, const int32_t* shard_index, int shard_count,
                          int total_count, char* all_text, void* stream);

#if defined(DSMI_BUILD) && defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* DSMI_H */
