/* spmx -- C ABI of the MI355X batch tokenization engine (libspmx.so).
 *
 * Drop-in boundary for ONE path of google/sentencepiece: text -> token ids
 * (normalize -> unigram Viterbi / BPE merge -> id post-processing).  Plain
 * pointers and sizes only; no C++ or torch types cross this boundary.
 *
 * Every entry point names the reference interface it replaces (paths relative
 * to the reference tree).  Return values are util::StatusCode numbers
 * (src/sentencepiece_processor.h:34-52): 0 = OK, 13 = INTERNAL, ...; the text
 * of the last error is available from spmx_last_error().  No C++ exception
 * crosses the boundary, as in the reference (only Status values).
 *
 * Thread safety: like SentencePieceProcessor's const methods, a loaded handle
 * may be used for encoding / decoding from several host threads at once: every
 * call leases its own workspace and stream, so the calls overlap on the GPU.
 * The mutators (set_encode_extra_options, set_vocabulary,
 * override_normalizer_spec, ...) must not race with them, as in the reference.  spmx_last_error() is per calling thread.
 */
#ifndef SPMX_H_
#define SPMX_H_
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct spmx_handle spmx_handle;

/* ---- load ---------------------------------------------------------------
 * SentencePieceProcessor::LoadFromSerializedProto(serialized)
 *   (src/sentencepiece_processor.h:261, .cc:234-240) followed by the Load()
 *   body (.cc:242-281): model factory (unigram | bpe), normalizer, prefix
 *   matcher.  The model's tables are compiled into the device layout and
 *   uploaded to GPU `device` (hip device ordinal).  Fails loudly (UNAVAILABLE)
 *   when no HIP device is usable: there is no CPU fallback. */
int spmx_create(const void *model_bytes, uint64_t n_bytes, int device, spmx_handle **out);
/* SentencePieceProcessor::Load(filename) (src/sentencepiece_processor.h:245). */
int spmx_create_from_file(const char *filename, int device, spmx_handle **out);
void spmx_destroy(spmx_handle *h);

/* util::Status::ToString() of the calling thread's last failing call (h is ignored and may be NULL). */
const char *spmx_last_error(const spmx_handle *h);

/* ---- configuration ------------------------------------------------------
 * SetEncodeExtraOptions("bos:eos:reverse") (src/sentencepiece_processor.h:267). */
int spmx_set_encode_extra_options(spmx_handle *h, const char *options);
/* SetDecodeExtraOptions("bos:eos:reverse") (src/sentencepiece_processor.h:270, .cc:288-291): applied to the pieces of
 * every later Decode before they are turned into text (.cc:819).  Same option syntax and error text as the encode side. */
int spmx_set_decode_extra_options(spmx_handle *h, const char *options);
/* SetVocabulary / ResetVocabulary (src/sentencepiece_processor.h:279-283). */
int spmx_set_vocabulary(spmx_handle *h, const char *const *pieces, const uint64_t *piece_lens, uint64_t n);
int spmx_reset_vocabulary(spmx_handle *h);
/* SentencePieceTrainer::SetProtoField(name, value, NormalizerSpec*) (src/spec_parser.h:256-270) applied to
 * mutable_normalizer_spec() (src/sentencepiece_processor.h:699), n pairs in the given order: what the Python wrapper's
 * OverrideNormalizerSpec(**kwargs) does (python/src/sentencepiece/sentencepiece.i:706-716, :1213-1217).
 *   fields    add_dummy_prefix, remove_extra_whitespaces, escape_whitespaces: booleans as string_util::lexical_cast<bool>
 *             reads them (src/util.h:60-77): 1 t true y yes / 0 f false n no, in any letter case; an empty value is true.
 *             name, normalization_rule_tsv: kept in the ModelProto only; they do not change what is encoded, as in the
 *             reference.  precompiled_charsmap: bytes (value_lens counts; a NULL value_lens means C strings throughout).
 *             The reference leaves its normalizer reading a freed string after this edit (src/normalizer.cc:47-68), so
 *             there is nothing to be equal to; here the invariant below defines it.
 *   errors    an unknown field: NOT_FOUND (5) `unknown field name "X" in NormalizerSpec.`; an unparsable boolean:
 *             INVALID_ARGUMENT (3) `cannot parse "V" as bool.`  The pairs before the failing one are applied, as the
 *             reference's loop leaves them; that pair and the ones behind it are not.  A charsmap that spmx_create would
 *             refuse gives spmx_create's error and changes nothing.
 * INVARIANT: after any sequence of calls the handle behaves like one newly created from its own spmx_serialized_model()
 * bytes -- the ModelProto it was loaded from with only the overridden normalizer_spec fields changed (an overridden
 * field is written explicitly, also at its default, as set_x() leaves the has-bit; every other byte is kept) -- under the
 * same SetVocabulary restriction, encode and decode extra options and profiling switch, all of which stay.  The self-test
 * samples are not run again (nor does the reference run them).
 * One call compiles and uploads the model's tables ONCE, however many pairs it carries -- what spmx_create costs without
 * the parse and the self-test -- and not at all when every field keeps its value.  The new tables are built beside the
 * old ones: if that fails (host or device memory, a bad charsmap) the handle keeps working on its previous spec.
 * spmx_handle_info reports the new table bytes.
 * Threading: as spmx_set_vocabulary.  It must not run while another call on the handle is in flight; before and after
 * such calls it is safe, from any thread. */
int spmx_override_normalizer_spec(spmx_handle *h, const char *const *fields, const char *const *values,
                                  const uint64_t *value_lens, uint64_t n);
/* model_proto().normalizer_spec()'s three switches as the handle applies them now (any pointer may be NULL). */
int spmx_normalizer_spec(const spmx_handle *h, int *add_dummy_prefix, int *remove_extra_whitespaces, int *escape_whitespaces);

/* ---- vocabulary accessors (src/sentencepiece_processor.h:638-677) -------- */
int spmx_piece_size(const spmx_handle *h);                                  /* GetPieceSize */
int spmx_piece_to_id(const spmx_handle *h, const char *piece, uint64_t len);/* PieceToId */
/* IdToPiece: copies up to cap bytes, returns the piece length (or -1). */
int64_t spmx_id_to_piece(const spmx_handle *h, int id, char *out, uint64_t cap);
int spmx_unk_id(const spmx_handle *h);
/* SentencePiece::Type of a piece (src/sentencepiece_model.proto:296-303): 1 NORMAL, 2 UNKNOWN, 3 CONTROL,
 * 4 USER_DEFINED, 5 UNUSED, 6 BYTE -- IsUnknown / IsControl / IsUnused / IsByte (sentencepiece_processor.h:653-662);
 * -1 for an id out of range. */
int spmx_piece_type(const spmx_handle *h, int id);
int spmx_bos_id(const spmx_handle *h);
int spmx_eos_id(const spmx_handle *h);
int spmx_pad_id(const spmx_handle *h);
int spmx_model_type(const spmx_handle *h);   /* trainer_spec.model_type: 1 unigram, 2 bpe, 3 word, 4 char */
/* Diagnostic: the kNf* bits the table compiler derived for this model (csrc/dev.h): which normalizer switches are on,
 * whether the one-byte space symbol / the word-wise BPE form apply. */
uint32_t spmx_model_flags(const spmx_handle *h);
/* trainer_spec.unk_piece (src/sentencepiece_model.proto:220), the string the `unk_piece` extra option writes
 * (src/sentencepiece_processor.cc:1050-1058): copies up to cap bytes, returns its length. */
int64_t spmx_unk_piece(const spmx_handle *h, char *out, uint64_t cap);

/* ---- encode -------------------------------------------------------------
 * All three are element-wise identical to calling
 *   SentencePieceProcessor::Encode(input, std::vector<int>* ids)
 *     (src/sentencepiece_processor.h:299-300, .cc:392-403)
 * per sentence, which is what the reference's only batch form --
 *   _EncodeAsIdsBatch (python/src/sentencepiece/sentencepiece.i:439-446) --
 * computes with a thread pool.
 *
 * No length limits: a sentence of any size is encoded (the fast kernels take what fits their length classes; what
 * does not -- documents, words of thousands of characters, BPE models whose pieces span words -- runs in kernels
 * whose working set lives in HBM, sized from the sentence).  The only bound is the reference's own int arithmetic:
 * the NORMALIZED form of one sentence must stay below 2^31 bytes.
 *
 * Per-sentence status: a sentence the reference's Encode would fail (kInternal "all normalized characters are not
 * consumed", e.g. a CONTROL piece among BPE symbols), or one beyond the bound above (OUT_OF_RANGE), yields NO ids;
 * the other sentences of the batch are unaffected -- what the reference's batch form does, whose workers call
 * EncodeAsIds and drop the Status (python/src/sentencepiece/sentencepiece.i:249-265).  The batch calls return OK;
 * the _ex forms report a util::StatusCode byte per sentence (0 = OK) and the number of failed sentences.
 *
 * Sentences are passed packed: `text` holds the bytes of all sentences back to
 * back, offsets[i] .. offsets[i+1] delimit sentence i (n + 1 entries).
 * Ids come back as CSR: ids[id_offsets[i] .. id_offsets[i+1]). */

/* Device-resident form: every pointer is HIP device memory on the handle's
 * GPU; `stream` is a hipStream_t (NULL = default stream).  The call enqueues
 * its kernels on `stream`, waits for them, and returns the number of ids in
 * *total_ids.  If ids_capacity is too small, returns RESOURCE_EXHAUSTED (8)
 * with the required capacity in *total_ids (id_offsets is still valid).
 * d_text may have any alignment; the kernels read it in ALIGNED 16-byte units, so the bytes that share a unit with the
 * text's first or last byte may be read (never interpreted) -- a unit does not cross a page, and a device allocation
 * covers whole pages. */
int spmx_encode_batch_device(spmx_handle *h, const void *d_text, uint64_t text_bytes, const uint64_t *d_offsets,
                             uint64_t n, int32_t *d_ids, uint64_t ids_capacity, uint64_t *d_id_offsets, void *stream,
                             uint64_t *total_ids);

/* As above, plus d_status (nullable): n status bytes in device memory; *n_failed (nullable): sentences with a
 * non-zero status. */
int spmx_encode_batch_device_ex(spmx_handle *h, const void *d_text, uint64_t text_bytes, const uint64_t *d_offsets,
                                uint64_t n, int32_t *d_ids, uint64_t ids_capacity, uint64_t *d_id_offsets,
                                uint8_t *d_status, void *stream, uint64_t *total_ids, uint64_t *n_failed);

/* Host-buffer form: copies text to the GPU, encodes, copies ids back.  Big batches (from 2^19 sentences) run as a
 * chunk pipeline on several host threads: staging copy, H2D, kernels and D2H of different chunks overlap.
 * *ids (total ids) and *id_offsets (n + 1) are allocated by the library and
 * released with spmx_free(). */
int spmx_encode_batch(spmx_handle *h, const char *text, const uint64_t *offsets, uint64_t n, int32_t **ids,
                      uint64_t **id_offsets);
/* As above, plus *status (nullable): n status bytes, released with spmx_free(); *n_failed (nullable). */
int spmx_encode_batch_ex(spmx_handle *h, const char *text, const uint64_t *offsets, uint64_t n, int32_t **ids,
                         uint64_t **id_offsets, uint8_t **status, uint64_t *n_failed);
/* The same batch given as n (pointer, length) pairs -- the layout of a std::vector<absl::string_view>'s elements as
 * this struct spells them: no packed copy is made, the sentences are gathered into the staging buffers chunk by chunk. */
typedef struct spmx_view { const char *data; uint64_t len; } spmx_view;
int spmx_encode_batch_views(spmx_handle *h, const spmx_view *views, uint64_t n, int32_t **ids, uint64_t **id_offsets,
                            uint8_t **status, uint64_t *n_failed);
/* One batch over several GPUs of the node from ONE process: handles[g] = the same model on GPU g.  The chunks of the
 * batch go round-robin over the GPUs (several in flight on each) and all land in ONE output CSR; no collective (the
 * multi-process form with an RCCL all-gather of the ids is sentencepiece_amd/sharding.py). */
int spmx_encode_batch_multi(spmx_handle *const *handles, int n_handles, const char *text, const uint64_t *offsets, uint64_t n,
                            int32_t **ids, uint64_t **id_offsets, uint8_t **status, uint64_t *n_failed);
void spmx_free(void *p);

/* ---- multi-GPU, one process per GPU: the ids of every rank on every rank, over RCCL ----------------------------------
 * The reference has no multi-device form; BASELINE.json's north_star asks for "a RCCL all-gatherv of the token-id output
 * over xGMI" behind the batch semantics of python/src/sentencepiece/sentencepiece.i:245-267 (the job's sentences in order,
 * each with its own ids).  Every rank encodes its contiguous shard of the job's sentences with
 * spmx_encode_batch_device and then calls spmx_all_gather_ids with its CSR; every rank gets the job's CSR:
 *   d_all_ids[rank_ids[r] ...)            rank r's ids (rank order = sentence order),
 *   d_all_id_offsets[0 .. total + 1)      offsets into d_all_ids, rebased to the whole job.
 * nccl_comm: the caller's ncclComm_t (one rank per GPU), or one made by spmx_rccl_comm_init.  librccl is looked up at the
 * first call (SPMX_RCCL_LIB names another library), it is no link-time dependency of libspmx.so.  d_scratch:
 * spmx_gather_scratch_words(world) uint64 of device memory (today 5 * (1 + world); ask, do not hard-code).  rank_sentences / rank_ids (host, world + 1 entries each, nullable): prefix sums over the
 * ranks.  Stream-ordered except for one read-back of the counts; collective: every rank of the communicator calls it.
 * Returns 0, or a util::StatusCode number (8: a capacity is too small -- the message names what is needed; 14: RCCL is
 * not loadable) with the text in spmx_gather_last_error().  Whether the gathered CSR fits is decided from EVERY rank's
 * capacities (they travel with the counts): when one rank's buffers are too small, all ranks return 8 and none starts a
 * transfer -- the ranks may size their buffers independently and retry together. */
int spmx_all_gather_ids(void *nccl_comm, int rank, int world, const int32_t *d_ids, uint64_t n_ids,
                        const uint64_t *d_id_offsets, uint64_t n_sentences, int32_t *d_all_ids, uint64_t all_ids_capacity,
                        uint64_t *d_all_id_offsets, uint64_t all_offsets_capacity, uint64_t *d_scratch,
                        uint64_t *rank_sentences, uint64_t *rank_ids, void *stream);
/* uint64 words of device scratch spmx_all_gather_ids needs for `world` ranks (0 for a world outside 1 .. 64). */
uint64_t spmx_gather_scratch_words(int world);
/* A communicator without linking RCCL oneself: rank 0 makes the 128-byte id and hands it to the other ranks by whatever
 * means the job has (a file, MPI, a socket); every rank then calls spmx_rccl_comm_init with its GPU current. */
int spmx_rccl_unique_id(void *id128);
int spmx_rccl_comm_init(void **nccl_comm, int world, int rank, const void *id128);
int spmx_rccl_comm_destroy(void *nccl_comm);
const char *spmx_gather_last_error(void);

/* ---- the packed gather: the same result from 16-bit ids and byte counts, with no host synchronisation per step ---------
 * spmx_all_gather_ids above moves int32 ids and uint64 offsets and reads the counts back in every call.  This form agrees
 * capacities ONCE (spmx_gather_plan_create, collective, the only place that synchronises), and then every step is
 * pack kernel -> transfer of equal-sized blocks -> unpack kernel, all stream-ordered: the number of ids is read on the device,
 * errors are found on the device and wait there until spmx_gather_plan_status asks.
 *
 * WIRE BLOCK, version 1 (one per rank; little endian; every section starts at a multiple of 128 bytes that follows from the
 * agreed capacities alone, so all blocks of a plan have one size and one layout -- spmx_packed_block_bytes):
 *   header  16 uint64: [0] 1 | 0x58504B31 << 32 (format version, magic)   [1] sentences   [2] ids
 *           [3] id width (2: piece_size <= 65536, else 4) | count width << 8 (1: max_ids_per_sentence <= 255, 2: <= 65535, else 4)
 *           [4] status bits, 0 = valid: 1 sentences over the agreed capacity, 2 ids over it, 4 a count outside the count
 *               width, 8 an id outside the id width, 16 a null buffer with a non-zero size.  A block with a status carries NO
 *               sentences: [1] / [2] then say what the sender was asked to pack, the payload is undefined.
 *           [5] [6] capacities of the sender's own d_all_ids / d_all_id_offsets   [7] [8] the agreed max_sentences / max_ids
 *   bases   per tile of 256 sentences the rank-local id offset at the tile's start, uint64: the receiver rebuilds the offsets
 *           of a tile from this and a scan over the tile's 256 counts alone
 *   counts  ids per sentence, count-width bytes each
 *   ids     id-width bytes each
 * Header, bases and alignment cost at most max_sentences / 32 + 520 bytes.  A block is padded to the agreed capacities and
 * travels whole: agree TIGHT capacities (byte-balanced shards differ by a few per cent; a capacity of twice the need doubles
 * the traffic).  A later version (a code shorter than 16 bits per id) announces itself in header word 0.
 *
 * Status of a gather (d_status of spmx_unpack_ids; inside a plan): 4 uint64 -- [0] 0 or the StatusCode number (8: a shard
 * over the agreed capacity, or the gathered CSR over some rank's output capacity; 11: a count or an id outside its width;
 * 3: a null buffer; 13: not a block of this version and these capacities), [1] the rank it names (0xFFFFFFFF: the caller's
 * own output buffers, spmx_unpack_ids only), [2] the status bits (32: output capacity, 64: format), [3] ids in the valid
 * blocks.  With a non-zero status the unpack writes NOTHING else: not the CSR, not the prefix sums.  Every rank decides from
 * the same world headers, so every rank gets the same answer and none is left waiting in a transfer. */
typedef struct spmx_gather_plan spmx_gather_plan;
/* Collective, ONCE: agrees MAX over the ranks of max_sentences, max_ids, max_ids_per_sentence and piece_size (one all-gather
 * of four words, read back), allocates world blocks on the current device.  Host-side errors (3, 13, 14) as above. */
int spmx_gather_plan_create(void *nccl_comm, int rank, int world, uint32_t piece_size, uint64_t max_sentences,
                            uint64_t max_ids, uint64_t max_ids_per_sentence, spmx_gather_plan **plan);
uint64_t spmx_gather_plan_block_bytes(const spmx_gather_plan *plan);
/* Stream-ordered, collective.  d_ids / d_id_offsets: the rank's CSR as spmx_encode_batch_device wrote it (the ids of the
 * shard are d_ids[d_id_offsets[0] .. d_id_offsets[n_sentences])).  Outputs as spmx_all_gather_ids, except that the prefix
 * sums d_rank_sentences / d_rank_ids (world + 1 entries each, nullable) are DEVICE memory.  Returns 0 when everything was
 * queued (3 / 13 / 14: a host-side failure); what the device found is spmx_gather_plan_status's to tell.  No read-back, no
 * stream synchronisation: a caller overlaps the gather with the next encode by giving it a stream of its own. */
int spmx_all_gather_ids_packed(spmx_gather_plan *plan, const int32_t *d_ids, const uint64_t *d_id_offsets,
                               uint64_t n_sentences, int32_t *d_all_ids, uint64_t all_ids_capacity,
                               uint64_t *d_all_id_offsets, uint64_t all_offsets_capacity, uint64_t *d_rank_sentences,
                               uint64_t *d_rank_ids, void *stream);
/* Synchronises `stream` and returns the status of the last gather queued on it: 0, or the StatusCode with the rank named
 * in spmx_gather_last_error().  The same on every rank.  A plan stays usable after a failed gather. */
int spmx_gather_plan_status(spmx_gather_plan *plan, void *stream);
void spmx_gather_plan_destroy(spmx_gather_plan *plan);
/* The two halves on their own -- for hosts with a transport of their own (MPI, torch.distributed), and for device -> host
 * copies of ids at about half the bytes.  No RCCL, no communicator; the caller passes the agreed numbers to every call.
 * d_block / d_blocks: device memory aligned to 128 bytes, spmx_packed_block_bytes(...) bytes per rank, the blocks of
 * spmx_unpack_ids back to back in rank order.  all_ids_capacity / all_offsets_capacity of spmx_pack_ids: what this rank's
 * unpack outputs will hold (they travel in the header; UINT64_MAX where every rank sizes its outputs alike).  d_status: 4
 * uint64 of device memory, written by every unpack; spmx_packed_status(host copy of them) turns them into the StatusCode and
 * the message of spmx_gather_last_error().  Both calls are stream-ordered and never synchronise. */
uint64_t spmx_packed_block_bytes(uint32_t piece_size, uint64_t max_sentences, uint64_t max_ids, uint64_t max_ids_per_sentence);
int spmx_pack_ids(const int32_t *d_ids, const uint64_t *d_id_offsets, uint64_t n_sentences, uint32_t piece_size,
                  uint64_t max_sentences, uint64_t max_ids, uint64_t max_ids_per_sentence, uint64_t all_ids_capacity,
                  uint64_t all_offsets_capacity, void *d_block, void *stream);
int spmx_unpack_ids(const void *d_blocks, int world, uint32_t piece_size, uint64_t max_sentences, uint64_t max_ids,
                    uint64_t max_ids_per_sentence, int32_t *d_all_ids, uint64_t all_ids_capacity, uint64_t *d_all_id_offsets,
                    uint64_t all_offsets_capacity, uint64_t *d_rank_sentences, uint64_t *d_rank_ids, uint64_t *d_status,
                    void *stream);
int spmx_packed_status(const uint64_t *status4);

/* Single sentence, caller-provided buffer (Encode(input, &ids)): returns the sentence's own Status, as the
 * reference does.  RESOURCE_EXHAUSTED with the needed size in *n_ids if cap is too small. */
int spmx_encode(spmx_handle *h, const char *text, uint64_t len, int32_t *ids, uint64_t cap, uint64_t *n_ids);

/* ---- decode -------------------------------------------------------------
 * Element-wise identical to SentencePieceProcessor::Decode(const std::vector<int>& ids, std::string*)
 *   (src/sentencepiece_processor.h:311-312, .cc:761-925): control pieces vanish, the unknown piece becomes
 *   trainer_spec.unk_surface, byte pieces are reassembled into UTF-8 (a structurally invalid byte -> U+FFFD),
 *   U+2581 -> ' ', leading whitespace handled as the normalizer_spec asks.  An id outside [0, GetPieceSize())
 *   fails the call with OUT_OF_RANGE (11) "Invalid id: N"; a model with a denormalizer_spec has its rules applied to
 *   the decoded text (.cc:905-907).
 * Ids are CSR (as produced by the encode calls); text comes back packed with text_offsets (n + 1 entries). */

/* Device-resident form: every pointer is HIP device memory.  If text_capacity is too small (or d_text is NULL)
 * returns RESOURCE_EXHAUSTED (8) with the required capacity in *total_bytes (d_text_offsets is valid). */
int spmx_decode_batch_device(spmx_handle *h, const int32_t *d_ids, const uint64_t *d_id_offsets, uint64_t n, void *d_text,
                             uint64_t text_capacity, uint64_t *d_text_offsets, void *stream, uint64_t *total_bytes);
/* Decode from PIECES: Decode(const std::vector<std::string>& pieces, ...) (src/sentencepiece_processor.h:303-309,
 * .cc:761-769; python/src/sentencepiece/sentencepiece.i:547 _DecodePiecesBatch).  The caller maps every piece to its id
 * (spmx_piece_to_id); a piece that is NOT in the vocabulary -- PieceToId gives the unknown id for a string other than the
 * unknown piece's -- goes through as it is (.cc:784-790): it travels as the id -(k + 1) with its bytes
 * lit_bytes[lit_offsets[k], lit_offsets[k + 1]) (k < n_lit; at most 65535 bytes each).  Under a decode extra option `unk`
 * (spmx_decode_unk_option() != 0) the reference rewrites such a piece to the unknown piece first (.cc:1050-1058): the
 * caller then passes the unknown id instead.  Everything else as spmx_decode_batch. */
int spmx_decode_batch_pieces(spmx_handle *h, const int32_t *ids, const uint64_t *id_offsets, uint64_t n, const char *lit_bytes,
                             const uint64_t *lit_offsets, uint64_t n_lit, char **text, uint64_t **text_offsets);
int spmx_decode_unk_option(const spmx_handle *h);
/* GetScore(id) (src/sentencepiece_processor.h:650): the piece's score as the ModelProto holds it; 11 for an id out of range. */
int spmx_piece_score(const spmx_handle *h, int id, float *score);
/* serialized_model_proto() (src/sentencepiece_processor.h:694): the bytes the handle was created from, with the overrides of
 * spmx_override_normalizer_spec patched in; owned by the handle, valid until the next override or spmx_destroy. */
int spmx_serialized_model(const spmx_handle *h, const char **data, uint64_t *n_bytes);
/* Host-buffer form; *text (total bytes) and *text_offsets (n + 1) are released with spmx_free(). */
int spmx_decode_batch(spmx_handle *h, const int32_t *ids, const uint64_t *id_offsets, uint64_t n, char **text,
                      uint64_t **text_offsets);
/* Single sentence, caller-provided buffer (Decode(ids, &text)); RESOURCE_EXHAUSTED with the needed size in *len. */
int spmx_decode(spmx_handle *h, const int32_t *ids, uint64_t n_ids, char *out, uint64_t cap, uint64_t *len);

/* ---- decode, SentencePieceText form -------------------------------------
 * What Decode(ids | pieces, SentencePieceText *) fills (src/sentencepiece_processor.cc:766-925), as arrays: the text, and
 * for every piece of the result its id and the byte range [begin, end) of its surface (SetSurface, .cc:822-828).
 *   The pieces of sentence s are the entries [piece_offsets[s], piece_offsets[s + 1]) (n + 1 offsets, the first 0), in the
 *   order after SetDecodeExtraOptions (.cc:819): reversed under `reverse`, the bos / eos ids in front / behind.
 *   Every piece has a range; a control piece an empty one at the text's length so far.  Of a character made of k byte
 *   pieces at offset o the first k - 1 get (o, o) and the last (o, o + k); an invalid byte piece gets U+FFFD, (o, o + 3).
 *   piece_ids: the ids as given, a piece outside the vocabulary (the pieces form) keeps its code -(k + 1).
 *   span_begin / span_end are uint32 byte offsets relative to the sentence's own text -- the text BEFORE the
 *   denormalizer: surface = raw_text[raw_offsets[s] + begin, raw_offsets[s] + end).  `text` is the text AFTER the
 *   denormalizer (.cc:905-907), what spmx_decode_batch returns; the spans are not rebased onto it.
 *   raw text: a model WITHOUT a denormalizer_spec has one text only.  The device form then writes neither d_raw_text nor
 *   d_raw_offsets (both may be NULL) and sets *raw_bytes = *total_bytes; the host forms set *raw_text and *raw_offsets to
 *   NULL.  The surfaces are slices of `text` in that case.
 * An id outside [0, GetPieceSize()) fails the call as in spmx_decode_batch and nothing is returned.
 *
 * Device-resident form.  Capacities: text_capacity bytes, piece_capacity entries in each of d_piece_ids / d_span_begin /
 * d_span_end, raw_capacity bytes; d_text_offsets, d_piece_offsets, d_raw_offsets hold n + 1 entries.  Returns
 * RESOURCE_EXHAUSTED (8) if one is too small: *total_pieces is always the number of pieces, *total_bytes / *raw_bytes the
 * bytes needed as far as the call got (a piece_capacity that is too small is reported before the denormalizer runs).  The
 * piece outputs are valid whenever piece_capacity sufficed, also if the text did not fit. */
int spmx_decode_batch_spans_device(spmx_handle *h, const int32_t *d_ids, const uint64_t *d_id_offsets, uint64_t n, void *d_text,
                                   uint64_t text_capacity, uint64_t *d_text_offsets, int32_t *d_piece_ids, uint32_t *d_span_begin,
                                   uint32_t *d_span_end, uint64_t piece_capacity, uint64_t *d_piece_offsets, void *d_raw_text,
                                   uint64_t raw_capacity, uint64_t *d_raw_offsets, void *stream, uint64_t *total_bytes,
                                   uint64_t *total_pieces, uint64_t *raw_bytes);
/* 1 if the model carries a denormalizer_spec with rules (the raw text outputs are then written), else 0. */
int spmx_has_denormalizer(const spmx_handle *h);
/* Host-array form; every output is released with spmx_free(). */
int spmx_decode_batch_spans(spmx_handle *h, const int32_t *ids, const uint64_t *id_offsets, uint64_t n, char **text,
                            uint64_t **text_offsets, int32_t **piece_ids, uint32_t **span_begin, uint32_t **span_end,
                            uint64_t **piece_offsets, char **raw_text, uint64_t **raw_offsets);
/* The pieces form: ids and literals as spmx_decode_batch_pieces takes them.  The surface of a literal is its own bytes. */
int spmx_decode_batch_pieces_spans(spmx_handle *h, const int32_t *ids, const uint64_t *id_offsets, uint64_t n,
                                   const char *lit_bytes, const uint64_t *lit_offsets, uint64_t n_lit, char **text,
                                   uint64_t **text_offsets, int32_t **piece_ids, uint32_t **span_begin, uint32_t **span_end,
                                   uint64_t **piece_offsets, char **raw_text, uint64_t **raw_offsets);

/* ---- spans form ---------------------------------------------------------
 * The ids plus, for every id, the byte range [begin, end) of its sentence that it covers: pieces(i).begin() /
 * .end() of the SentencePieceText that Encode(absl::string_view, SentencePieceText *) fills
 * (src/sentencepiece_processor.cc:638-651, PopulateSentencePieceText :547-636, bos / eos spans :1029-1048).
 * Offsets are relative to the start of the sentence, in bytes (the C++ convention; the Python wrapper converts to
 * characters, sentencepiece.i ConvertToUnicodeSpans).  surface = input[begin, end); the piece of a known id is
 * IdToPiece(id).  Offsets are 32-bit: sentences below 4 GiB.
 * nbegin / nend (optional, both or neither): the same tokens as byte ranges of the NORMALIZED sentence
 * (spmx_normalize_batch): the piece of an unknown token is that text (:614-617); 0, 0 for a bos / eos.
 * d_begin / d_end / d_nbegin / d_nend: ids_capacity entries each; the arrays of the host form are released with
 * spmx_free(). */
int spmx_encode_batch_spans_device(spmx_handle *h, const void *d_text, uint64_t text_bytes, const uint64_t *d_offsets,
                                   uint64_t n, int32_t *d_ids, uint64_t ids_capacity, uint64_t *d_id_offsets,
                                   uint32_t *d_begin, uint32_t *d_end, uint32_t *d_nbegin, uint32_t *d_nend, void *stream,
                                   uint64_t *total_ids);
int spmx_encode_batch_spans(spmx_handle *h, const char *text, const uint64_t *offsets, uint64_t n, int32_t **ids,
                            uint64_t **id_offsets, uint32_t **begin, uint32_t **end, uint32_t **nbegin, uint32_t **nend);
/* As above, plus *status (nullable): n status bytes, released with spmx_free(); *n_failed (nullable): what
 * Encode(input, SentencePieceText *) returns per sentence (src/sentencepiece_processor.cc:638-651 -> :628). */
int spmx_encode_batch_spans_ex(spmx_handle *h, const char *text, const uint64_t *offsets, uint64_t n, int32_t **ids,
                               uint64_t **id_offsets, uint32_t **begin, uint32_t **end, uint32_t **nbegin, uint32_t **nend,
                               uint8_t **status, uint64_t *n_failed);
/* The message of a per-sentence status byte (the _ex forms): for INTERNAL (13) the reference's "all normalized
 * characters are not consumed." (src/sentencepiece_processor.cc:628); "" for 0. */
const char *spmx_status_message(int code);

/* ---- batch Normalize ----------------------------------------------------
 * SentencePieceProcessor::Normalize(input, &normalized, &norm_to_orig) (src/sentencepiece_processor.cc:933-945 ->
 * Normalizer::Normalize, src/normalizer.cc:71-186) per sentence: the packed normalized text + n + 1 offsets and,
 * optionally, the alignment vectors: sentence s owns entries [norm_offsets[s] + s, norm_offsets[s + 1] + s + 1) of
 * norm_to_orig -- one per normalized byte plus the closing one, which is 0xFFFFFFFF where the reference's vector
 * is empty (empty or all-whitespace input).  No length limit (OUT_OF_RANGE only where the normalized form of a
 * sentence would exceed 2^31 bytes).
 * Device form: d_norm_to_orig (nullable) holds norm_capacity + n + 1 entries. */
int spmx_normalize_batch_device(spmx_handle *h, const void *d_text, const uint64_t *d_offsets, uint64_t n, void *d_norm,
                                uint64_t norm_capacity, uint64_t *d_norm_offsets, uint32_t *d_norm_to_orig, void *stream,
                                uint64_t *total_bytes);
int spmx_normalize_batch(spmx_handle *h, const char *text, const uint64_t *offsets, uint64_t n, char **norm,
                         uint64_t **norm_offsets, uint32_t **norm_to_orig);

/* ---- n-best -------------------------------------------------------------
 * NBestEncode(input, nbest_size, std::vector<std::vector<int>>*) (src/sentencepiece_processor.h:323-324;
 * unigram::Model::NBestEncode src/unigram_model.cc:686-717, Lattice::NBest :345-515) per sentence, unigram models
 * only (INTERNAL otherwise, as the reference).  nbest_size is clamped to [1, 1024]; 1 is the plain encoder with
 * score 0.  Result r of the batch: ids[id_offsets[r], id_offsets[r + 1]) and scores[r]; sentence s owns the
 * results [result_offsets[s], result_offsets[s + 1]) (n + 1 entries), best first.  The four arrays are released
 * with spmx_free().  No length limit: a sentence beyond the first launch's lattice capacities (1024 normalized bytes,
 * 16384 nodes) runs in a second launch sized for it; RESOURCE_EXHAUSTED only where the device memory for one
 * sentence's lattice and agenda runs out. */
int spmx_nbest_encode_batch(spmx_handle *h, const char *text, const uint64_t *offsets, uint64_t n, int nbest_size,
                            int32_t **ids, uint64_t **id_offsets, float **scores, uint64_t **result_offsets);
/* NBestEncode(input, nbest_size, NBestSentencePieceText *) / (…, std::vector<std::vector<std::string>> *)
 * (src/sentencepiece_processor.h:318-324, .cc:653-676): the same results, plus for every id of every result the byte
 * range of the input (begin / end) and of the normalized text (nbegin / nend) its piece covers -- the four arrays of
 * the spans form above, indexed like ids; released with spmx_free().  A run of unknown characters is one piece; of a
 * character's byte-fallback pieces the last carries the range (sentencepiece_processor.cc:581-617). */
int spmx_nbest_encode_batch_spans(spmx_handle *h, const char *text, const uint64_t *offsets, uint64_t n, int nbest_size,
                                  int32_t **ids, uint64_t **id_offsets, float **scores, uint64_t **result_offsets,
                                  uint32_t **begin, uint32_t **end, uint32_t **nbegin, uint32_t **nend);

/* ---- sampling and the original encoder -----------------------------------
 * SampleEncode(input, nbest_size, alpha, std::vector<int>*) (src/sentencepiece_processor.h:346-353, .cc:678-720) per
 * sentence, the subword-regularization entry:
 *   unigram models (IsNBestEncodeAvailable):
 *     nbest_size < 0      one segmentation drawn from the lattice, Lattice::Sample(alpha) (forward filtering /
 *                         backward sampling, src/unigram_model.cc:511-542)
 *     nbest_size 0 or 1   the plain encoder
 *     nbest_size > 1      one of the nbest_size best, drawn with probability ~ exp(alpha * score) (:700-716)
 *   BPE models: EVERY nbest_size is BPE-dropout with merge-skip probability alpha (.cc:688-693 sends the call to
 *     bpe::Model::SampleEncode, src/bpe_model.cc:131-156); alpha <= 0 is the plain encoder
 *   nbest_size > 512    INTERNAL "nbest_size must be nbest_size <= 512" (.cc:684)
 * Draws come from generators keyed by (seed, sentence index) -- reproducible per call; the reference's thread-local
 * mt19937 stream is not (and cannot be) reproduced, its own tests pin the DISTRIBUTION (unigram_model_test.cc:429-470,
 * bpe_model_test.cc:252-295), as tests/test_sampling.py does.  alpha = 0 under BPE is bit-equal to Encode. */
int spmx_sample_encode_batch(spmx_handle *h, const char *text, const uint64_t *offsets, uint64_t n, int nbest_size,
                             float alpha, uint64_t seed, int32_t **ids, uint64_t **id_offsets);
/* SampleEncode(input, nbest_size, alpha, SentencePieceText *) / (…, std::vector<std::string> *)
 * (src/sentencepiece_processor.h:346-353, :404-408): the drawn segmentation with the four span arrays (as above). */
int spmx_sample_encode_batch_spans(spmx_handle *h, const char *text, const uint64_t *offsets, uint64_t n, int nbest_size,
                                   float alpha, uint64_t seed, int32_t **ids, uint64_t **id_offsets, uint32_t **begin,
                                   uint32_t **end, uint32_t **nbegin, uint32_t **nend);
/* ---- lattice scoring -------------------------------------------------------
 * CalculateEntropy(input, alpha, float *) (src/sentencepiece_processor.h:385-386, .cc:748-759; Lattice::CalculateEntropy
 * src/unigram_model.cc:263-291) per sentence, unigram models only (INTERNAL "CalculateEntropy is not available for the
 * current model." otherwise): *entropy holds n floats, released with spmx_free().  The value is the REFERENCE's: its
 * float recurrences in its order, which on long text lie far from the exact entropy.  An empty
 * sentence gives -0.0, as the reference does.  No length limit. */
int spmx_calculate_entropy_batch(spmx_handle *h, const char *text, const uint64_t *offsets, uint64_t n, float alpha,
                                 float **entropy);
/* SampleEncodeAndScore(input, num_samples, alpha, wor, include_best, ...) (src/sentencepiece_processor.h:355-378,
 * .cc:724-746; unigram::Model::SampleEncodeAndScore src/unigram_model.cc:741-846) per sentence, unigram models only
 * (INTERNAL "SampleEncodeAndScore is not available for the current model." otherwise).  Results as
 * spmx_nbest_encode_batch gives them.
 *   wor = 0   num_samples segmentations drawn independently from the lattice (Lattice::Sample(alpha)), each with
 *             score = log of its probability: the float sum of alpha * piece score minus the lattice's log Z.
 *             Draw j of sentence i comes from a generator keyed by (seed, i, j) alone.
 *   wor = 1   num_samples DISTINCT segmentations by Gumbel top-k (Lattice::NBest(num_samples + 1, true, alpha),
 *             src/unigram_model.cc:391-450): the search's last result gives the threshold kappa and is dropped, and a
 *             score is the log of the segmentation's inclusion probability (:811-826).  include_best puts the Viterbi
 *             path first, with score 0.0, and takes it out of the samples (:775-793).  A lattice with P <= num_samples
 *             paths gives P - 1 results, as the reference does.  The Gumbel variates come from a generator keyed by
 *             (seed, sentence index).
 * The seed goes through a 64-bit hash before it enters either key: seed and seed + 1 give unrelated draws, so callers
 * may simply count up (the hosts do, for calls without a seed of their own).
 * A sentence that is empty after normalization owns no result, nor does, without replacement, one whose lattice has a
 * single path: the reference's per-sentence INTERNAL "SampleEncodeAndScore returns empty result." (.cc:735).  The call
 * fails with that status where no sentence could own one: include_best without wor, num_samples < 1.  num_samples > 512 is refused with INTERNAL (the 0.2.1 sources
 * have no cap). */
int spmx_sample_encode_and_score_batch(spmx_handle *h, const char *text, const uint64_t *offsets, uint64_t n,
                                       int num_samples, float alpha, int wor, int include_best, uint64_t seed,
                                       int32_t **ids, uint64_t **id_offsets, float **scores, uint64_t **result_offsets);
/* ... with the four span arrays of spmx_nbest_encode_batch_spans. */
int spmx_sample_encode_and_score_batch_spans(spmx_handle *h, const char *text, const uint64_t *offsets, uint64_t n,
                                             int num_samples, float alpha, int wor, int include_best, uint64_t seed,
                                             int32_t **ids, uint64_t **id_offsets, float **scores,
                                             uint64_t **result_offsets, uint32_t **begin, uint32_t **end,
                                             uint32_t **nbegin, uint32_t **nend);

/* ---- the lattice calls on device buffers ------------------------------------
 * NBestEncode with the text and every result on the device: the search as spmx_nbest_encode_batch runs it, then its sparse
 * results go to a dense CSR on the device (kernels_latticecsr.h) -- nothing but a few counters crosses to the host.  Input
 * as spmx_encode_batch_device.  Output, the rows spmx_nbest_encode_batch returns, in the caller's device memory: sentence s
 * owns the results [d_result_offsets[s], d_result_offsets[s + 1]) (n + 1 entries), best first; result r is
 * d_ids[d_id_offsets[r], d_id_offsets[r + 1]) with d_scores[r], and d_sent_of_result[r] (may be NULL) is its sentence.
 * d_id_offsets holds results_capacity + 1 entries, d_scores and d_sent_of_result results_capacity.  The buffers may have
 * any alignment their element type allows.
 * Capacity protocol of spmx_encode_batch_pieces_device: too small a results_capacity or ids_capacity ->
 * RESOURCE_EXHAUSTED (8) with *total_results and *total_ids set and nothing written outside the buffers; NULL buffers with
 * capacity 0 ask for the sizes.  A model that is not unigram: INTERNAL "NBestEncode is not available for the current
 * model."; nbest_size 1 (and n == 0) is the plain encoder, score 0, one result per sentence. */
int spmx_nbest_encode_batch_device(spmx_handle *h, const void *d_text, uint64_t text_bytes, const uint64_t *d_offsets,
                                   uint64_t n, int nbest_size, int32_t *d_ids, uint64_t ids_capacity, uint64_t *d_id_offsets,
                                   float *d_scores, uint32_t *d_sent_of_result, uint64_t results_capacity,
                                   uint64_t *d_result_offsets, void *stream, uint64_t *total_results, uint64_t *total_ids);
/* SampleEncode on device buffers, every branch of spmx_sample_encode_batch: lattice sampling (nbest_size < 0), the plain
 * encoder (0 or 1), one of the nbest_size best drawn on the device (> 1), BPE-dropout for BPE models (alpha <= 0: the plain
 * encoder); the refusals are the host call's.  One result per sentence: d_id_offsets holds n + 1 entries.  The draws of
 * sentence s are keyed by (seed, index_base + s): sentences [k, n) of a batch, run with index_base = k, give the rows k..n
 * of the whole batch -- a corpus may be cut anywhere.  index_base 0 gives what spmx_sample_encode_batch gives, but for
 * nbest_size > 1, where a draw within one rounding of exp() of a boundary between two results may fall on the other side
 * (the device's exp against glibc's).  Capacity protocol as spmx_encode_batch_device. */
int spmx_sample_encode_batch_device(spmx_handle *h, const void *d_text, uint64_t text_bytes, const uint64_t *d_offsets,
                                    uint64_t n, int nbest_size, float alpha, uint64_t seed, uint64_t index_base,
                                    int32_t *d_ids, uint64_t ids_capacity, uint64_t *d_id_offsets, void *stream,
                                    uint64_t *total_ids);
/* SampleEncodeAndScore on device buffers: arguments and refusals of spmx_sample_encode_and_score_batch, outputs and
 * capacity protocol of spmx_nbest_encode_batch_device.  A sentence without a result owns an empty range. */
int spmx_sample_encode_and_score_batch_device(spmx_handle *h, const void *d_text, uint64_t text_bytes,
                                              const uint64_t *d_offsets, uint64_t n, int num_samples, float alpha, int wor,
                                              int include_best, uint64_t seed, int32_t *d_ids, uint64_t ids_capacity,
                                              uint64_t *d_id_offsets, float *d_scores, uint32_t *d_sent_of_result,
                                              uint64_t results_capacity, uint64_t *d_result_offsets, void *stream,
                                              uint64_t *total_results, uint64_t *total_ids);

/* The reference's ORIGINAL unigram encoder (EncoderVersion::kOriginal, src/unigram_model.cc:674-692): the lattice of
 * Lattice::SetSentence / Model::PopulateNodes and Lattice::Viterbi (:161-198, all-float, first best left node wins)
 * instead of EncodeOptimized.  Same ids except where float and double arithmetic break a tie differently. */
int spmx_encode_batch_original(spmx_handle *h, const char *text, const uint64_t *offsets, uint64_t n, int32_t **ids,
                               uint64_t **id_offsets);

/* ---- expected piece counts: the unigram trainer's E-step under the loaded model ----------------------------------------
 * What unigram::Trainer::RunEStep (src/unigram_model_trainer.cc:318-367) computes per training sentence, for a batch:
 * the lattice of Lattice::SetSentence / Model::PopulateNodes over the normalized sentence, Lattice::PopulateMarginal
 * (src/unigram_model.cc:235-261: forward, backward, exp(alpha + score + beta - Z) per node -- the reference's float
 * recurrences in its order) and the node count of Lattice::Viterbi().  Sentence s has the weight freq[s]
 * (NULL: 1).  Unknown characters are counted under unk_id; byte-fallback pieces never are (the marginal is a lattice
 * quantity).  Unigram models only: INTERNAL "ExpectedCounts is not available for the current model." otherwise.
 *
 * Counts are FIXED POINT with SPMX_EXPECTED_FRAC_BITS fraction bits: a node adds the integer
 * llrint(freq * p * 2^24) (to nearest, ties to even) to the 64-bit accumulator of its piece, so a result does not depend on
 * the launch shape, the order of the adds or where a corpus is cut into batches -- batches add up exactly.  Expected count
 * = acc / 2^24; a node is quantized by at most 2^-25; an accumulator holds 2^40 (about 1.1e12) weighted occurrences of a
 * piece before it wraps.
 *   log_z[s]          log Z of sentence s as a float, NOT multiplied by freq[s]; 0 for a sentence that is empty after
 *                     normalization (which adds nothing and has 0 nodes)
 *   viterbi_nodes[s]  nodes on the best path (Lattice::Viterbi, all-float), before any id rule: a run of unknown
 *                     characters counts one per character
 * No length limit.  n == 0 is valid. */
#define SPMX_EXPECTED_FRAC_BITS 24
/* device form: text, offsets, freq (nullable) on the device; d_acc[piece_size] is ADDED to; d_log_z / d_viterbi_nodes
   [n], nullable; stream-ordered apart from the synchronisations the lattice launches have (n == 0: nothing is touched) */
int spmx_expected_counts_batch_device(spmx_handle *h, const void *d_text, uint64_t text_bytes, const uint64_t *d_offsets,
                                      uint64_t n, const uint32_t *d_freq, unsigned long long *d_acc, float *d_log_z,
                                      uint32_t *d_viterbi_nodes, void *stream);
/* host form: expected[piece_size] doubles, OVERWRITTEN (= acc / 2^24, exact below 2^29); log_z / viterbi_nodes malloc'ed
   [n], released with spmx_free(), nullable */
int spmx_expected_counts_batch(spmx_handle *h, const char *text, const uint64_t *offsets, uint64_t n, const uint32_t *freq,
                               double *expected, float **log_z, uint32_t **viterbi_nodes);

/* ---- corpus packer ------------------------------------------------------
 * The caller-side step of the reference's spm_encode (src/spm_encode_main.cc:159-165: std::getline over the input
 * file, one Encode per line) on the device: a file image with '\n'-terminated lines -> the packed text (without
 * the terminators; '\r' is kept, as getline keeps it) + n_lines + 1 offsets that the encode calls take.  A last line
 * without '\n' counts; "a\n" is one line.  d_file must be 16-byte aligned device memory.  Too small a capacity ->
 * RESOURCE_EXHAUSTED (8) with the needed sizes in *n_lines (+ 1 offsets) and *text_bytes. */
int spmx_split_lines_device(spmx_handle *h, const void *d_file, uint64_t bytes, void *d_text, uint64_t text_capacity,
                            uint64_t *d_offsets, uint64_t offsets_capacity, void *stream, uint64_t *n_lines,
                            uint64_t *text_bytes);

/* ---- corpus file -> ids --------------------------------------------------
 * What the reference's `spm_encode --output_format=id < in > out` does (src/spm_encode_main.cc:115-119, :159-165: getline,
 * Encode, StrJoin(ids, " ")), as one call: the file is mmap'ed and goes through a pipeline of worker threads -- pinned
 * staging, H2D, the device line splitter, the encode kernels, the token-text kernels, one D2H of the finished image --
 * chunk by chunk (64 MiB, SPMX_FILE_CHUNK as in spmx_decode_file), in order.
 * format "id": the reference's text output, byte for byte; "piece": what `spm_encode` writes without a format flag
 * (--output_format=piece, :110-114: the pieces joined with ' '); "bin": out_path receives the ids (int32, flat) and
 * out_path + ".idx" the n + 1 uint64 offsets.  NULL: "id".  The encode extra options apply to every format.  A sentence
 * that fails by itself has no ids and becomes an empty line. */
int spmx_encode_file(spmx_handle *h, const char *in_path, const char *out_path, const char *format, uint64_t *n_sentences,
                     uint64_t *n_ids);
/* spmx_encode_file with the lattice formats of spm_encode (src/spm_encode_main.cc:120-153).  "id", "piece" and "bin" are
 * spmx_encode_file's, byte for byte.  "nbest_id" / "nbest_piece": NBestEncode(line, nbest_size) per input line, one output
 * line of ids / of pieces per result, best first (:136-149; unigram models only, INTERNAL otherwise as the reference).
 * "sample_id" / "sample_piece": SampleEncode(line, nbest_size, alpha) per input line, one output line (:122-131), every branch of
 * spmx_sample_encode_batch_device; the draws of a line are keyed by (seed, its line number in the file) alone, whatever
 * SPMX_FILE_CHUNK is and however many workers run, and equal spmx_sample_encode_batch's over the file's lines with the same
 * seed.  "proto", "sample_proto", "nbest_proto": the reference encodes and writes nothing; here out_path is left empty
 * without encoding.  Pieces are what NBestEncodeAsPieces / SampleEncodeAsPieces give, the encode extra options (bos, eos,
 * reverse, unk_piece) included.  *n_sentences counts input lines, *n_lines output lines, *n_ids the ids (pieces) written;
 * any of them may be NULL.  Ids and pieces reach the file through the device's token-text writer over the result CSR, one
 * D2H of the finished image per chunk. */
int spmx_encode_file_ex(spmx_handle *h, const char *in_path, const char *out_path, const char *format, int nbest_size,
                        float alpha, uint64_t seed, uint64_t *n_sentences, uint64_t *n_lines, uint64_t *n_ids);

/* ---- corpus file side of Decode ------------------------------------------
 * The caller-side steps of the reference's spm_decode (src/spm_decode_main.cc: std::getline, StrSplit(line, " ") without
 * empty tokens, atoi per token, Decode, WriteLine) on the device.
 *
 * Parser: a file image of id lines -> CSR ids.  Lines as in spmx_split_lines_device.  A token is a maximal run of bytes
 * other than ' ' within a line; an empty line, or one of spaces, has no ids.  A token's value is glibc's atoi, bit for
 * bit: leading \t \v \f \r, one sign, the digits up to the first other byte, strtol's saturation, the low 32 bits.
 * d_file must be 16-byte aligned device memory, its allocation padded to 16 bytes.  d_ids takes ids_capacity entries,
 * d_id_offsets offsets_capacity (n_lines + 1 are written).  Too small a capacity -> RESOURCE_EXHAUSTED (8) with the
 * needed sizes in *n_lines (+ 1 offsets) and *n_ids.  bytes == 0: an empty CSR (d_id_offsets[0] = 0). */
int spmx_parse_id_lines_device(spmx_handle *h, const void *d_file, uint64_t bytes, int32_t *d_ids, uint64_t ids_capacity,
                               uint64_t *d_id_offsets, uint64_t offsets_capacity, void *stream, uint64_t *n_lines,
                               uint64_t *n_ids);
/* Joiner, the inverse of spmx_split_lines_device: packed text + n + 1 offsets (d_text_offsets[0] == 0, as the decode
 * calls write them) -> a file image of d_text_offsets[n] + n bytes, every line followed by '\n'.  Too small a capacity
 * (or d_out NULL) -> RESOURCE_EXHAUSTED (8) with the needed size in *out_bytes.  d_out may have any alignment. */
int spmx_join_lines_device(spmx_handle *h, const void *d_text, const uint64_t *d_text_offsets, uint64_t n, void *d_out,
                           uint64_t out_capacity, void *stream, uint64_t *out_bytes);

/* ---- token text: the output side of spm_encode on the device ---------------
 * The inverse of the parser: CSR ids -> a file image of id lines, absl::StrJoin(ids, " ") + '\n' per line
 * (src/spm_encode_main.cc:116-119); a line without ids is a single '\n'.  Every int32 is written (a negative id with '-'),
 * so spmx_parse_id_lines_device of the image gives the CSR back.  Too small a capacity (or d_out NULL) ->
 * RESOURCE_EXHAUSTED (8) with the needed size in *out_bytes.  n == 0: an empty image.  d_out may have any alignment. */
int spmx_format_id_lines_device(spmx_handle *h, const int32_t *d_ids, const uint64_t *d_id_offsets, uint64_t n, void *d_out,
                                uint64_t out_capacity, void *stream, uint64_t *out_bytes);
/* EncodeAsPieces for a batch: text -> ids (as spmx_encode_batch_device) + the pieces' bytes back to back and their
 * *total_ids + 1 offsets.  A piece is the token's range of the normalized sentence -- an unknown token shows its
 * characters -- the name of a byte-fallback or control piece, or trainer_spec.unk_piece for an unknown token under the
 * encode extra option `unk` / `unk_piece` (src/sentencepiece_processor.cc:566-620, :1050-1058).  d_piece_offsets holds
 * ids_capacity + 1 entries.  Too small an ids_capacity -> RESOURCE_EXHAUSTED (8) with *total_ids (the piece bytes are
 * not counted then); too small a piece_bytes_capacity (or a NULL buffer) -> 8 with both totals. */
int spmx_encode_batch_pieces_device(spmx_handle *h, const void *d_text, uint64_t text_bytes, const uint64_t *d_offsets,
                                    uint64_t n, int32_t *d_ids, uint64_t ids_capacity, uint64_t *d_id_offsets,
                                    void *d_piece_bytes, uint64_t piece_bytes_capacity, uint64_t *d_piece_offsets,
                                    void *stream, uint64_t *total_ids, uint64_t *total_piece_bytes);
/* ... host-buffer form: the four arrays are malloc'ed here (spmx_free) */
int spmx_encode_batch_pieces(spmx_handle *h, const char *text, const uint64_t *offsets, uint64_t n, int32_t **ids,
                             uint64_t **id_offsets, char **piece_bytes, uint64_t **piece_offsets);
/* text -> piece lines: what spm_encode --output_format=piece writes for these sentences, the pieces of a sentence joined
 * with ' ' and followed by '\n' (an empty sentence: a single '\n').  Capacity protocol as spmx_format_id_lines_device;
 * *n_ids is the number of pieces. */
int spmx_encode_piece_lines_device(spmx_handle *h, const void *d_text, uint64_t text_bytes, const uint64_t *d_offsets,
                                   uint64_t n, void *d_out, uint64_t out_capacity, void *stream, uint64_t *n_ids,
                                   uint64_t *out_bytes);

/* ---- ids -> corpus file ---------------------------------------------------
 * What the reference's `spm_decode --input_format=id < in > out` does, as one call and as the inverse of
 * spmx_encode_file: the input is mmap'ed, cut at line ends into chunks of 64 MiB (SPMX_FILE_CHUNK, bytes, at least 4096:
 * read at every call) and goes through up to 4 worker threads -- H2D, the parser, the decode kernels, the joiner, one
 * D2H of the finished image, fwrite -- in order.  The decode extra options and a model's denormalizer apply.
 * input_format "id": lines of decimal ids; "bin": in_path holds flat int32 ids and in_path + ".idx" the n + 1 uint64
 * offsets (what spmx_encode_file's "bin" writes); "piece": lines of space-separated pieces, mapped with PieceToId on the
 * host -- a token outside the vocabulary goes through as it is, or becomes the unknown piece under the decode option
 * `unk`, as spmx_decode_batch_pieces documents.  NULL: "id".
 * An id outside [0, GetPieceSize()) fails the call with OUT_OF_RANGE (11) "Invalid id: N": of several failing chunks
 * the first one's status is returned, N being an invalid id of that chunk's first failing line.  What out_path holds
 * after a failed call is unspecified.  A missing input: NOT_FOUND (5). */
int spmx_decode_file(spmx_handle *h, const char *in_path, const char *out_path, const char *input_format, uint64_t *n_lines,
                     uint64_t *n_ids);

/* ---- piece frequency counts: spm_encode --generate_vocabulary --------------
 * The vocabulary workflow of the reference's spm_encode (src/spm_encode_main.cc:80-83, :102-109, :167-172): count how often
 * every piece is emitted over a corpus, write the counts as a vocabulary file, encode with the rare pieces switched off.
 * The reference counts piece strings in a map; piece strings are unique in a loaded model, so the counts are a histogram
 * over ids, filtered by piece type when the file is written.  The reference counts in `int`, the counts here are 64-bit:
 * the two agree while every count is below 2^31.
 *
 * The histogram kernel: d_ids[n_ids] (int32, device, any 4-byte alignment) -> d_counts[GetPieceSize() + 1] (uint64, device),
 * ADDED to what is there.  d_counts[id] for 0 <= id < GetPieceSize(); the last entry counts every other value.  The call
 * only enqueues on `stream`: no status word, no host synchronisation.  counts_capacity < GetPieceSize() + 1 (or d_counts
 * NULL) -> RESOURCE_EXHAUSTED (8), nothing is written.  n_ids == 0: nothing is enqueued. */
int spmx_count_ids_device(spmx_handle *h, const int32_t *d_ids, uint64_t n_ids, uint64_t *d_counts, uint64_t counts_capacity,
                          void *stream);
/* The histogram of a corpus file: the pipeline of spmx_encode_file (mmap, chunks at line ends, SPMX_FILE_CHUNK, up to 4
 * workers) with the histogram kernel in place of formatting.  Nothing comes back per chunk; the GetPieceSize() + 1 words
 * come back once and are ADDED to counts (host), so several files accumulate.  The encode extra options and a vocabulary
 * restriction apply; bos / eos, unknown and control ids are counted here (the raw histogram) and left out by
 * spmx_write_vocabulary.  Errors as spmx_encode_file. */
int spmx_count_file(spmx_handle *h, const char *in_path, uint64_t *counts, uint64_t *n_sentences, uint64_t *n_ids);
/* counts (host, GetPieceSize() + 1) -> the file `spm_encode --generate_vocabulary` writes: one line piece TAB count per
 * piece that occurred and is neither UNKNOWN nor CONTROL (BYTE and USER_DEFINED pieces are written), by descending count,
 * equal counts by ascending piece in unsigned byte order (Sorted, src/trainer_interface.h:36-50).  *n_lines: lines written. */
int spmx_write_vocabulary(spmx_handle *h, const uint64_t *counts, const char *out_path, uint64_t *n_lines);
/* LoadVocabulary (src/sentencepiece_processor.cc:341-362): lines "token TAB freq"; the tokens whose freq reaches `threshold`
 * (1 where the line has no second column) become the valid vocabulary (spmx_set_vocabulary: a character or word model
 * refuses).  A missing file: NOT_FOUND (5); an empty token or a frequency that does not parse: INTERNAL (13). */
int spmx_load_vocabulary(spmx_handle *h, const char *path, int threshold);

/* ---- measurement --------------------------------------------------------
 * Per-kernel timing of the encode kernels of the LAST profiled encode call on the handle, measured with hipEvents
 * on the call's stream (enable first).  Arrays hold 7 entries ("kernel slots": 0 the streaming launch over the
 * classes up to 16 KiB, 1 the streaming launch over the document classes, 2 the overflow launch, 3 the
 * sentence-per-wave BPE launches, 4 the long form (the wave-cooperative unigram form included), 5 the first round of the
 * word form, 6 its second round; unused slots are zero); returns the number of slots (callers size for 8).
 * spmx_last_profile_name() gives the kernel symbol of a slot as rocprofv3 prints it.  bytes[] is the algorithmic
 * byte count SURVEY.md section 8d defines (raw bytes + 8 + 4 * ids + 8 per sentence).  path[8]: sentences the main
 * tiles set aside on hard lists, sentences on the overflow list, sentences that took the long form, failed sentences,
 * times the call encoded the batch again because the id arena was too small, launches of the long form (slot 4),
 * wavefronts per workgroup of the word-per-lane form's first and of its second round (0: the round did not take that form). */
int spmx_set_profiling(spmx_handle *h, int enabled);
int spmx_last_profile_name(const spmx_handle *h, int slot, char *out, uint64_t cap);
int spmx_last_profile(const spmx_handle *h, float *kernel_ms, uint64_t *sentences, uint64_t *raw_bytes,
                      uint64_t *ids, uint64_t *bytes, uint64_t *path, float *total_ms);

/* Shader-clock cycles the waves of the LAST profiled call spent per phase, summed over waves:
 * cycles[5 * slot + {0 load, 1 normalize, 2 segment, 3 emit}] (35 entries; callers size for 40); entry 4 is the number of search-loop
 * iterations the waves of the lane-per-sentence forms executed. */
int spmx_last_phase_cycles(const spmx_handle *h, uint64_t *cycles);

/* What loading this handle cost: the device bytes of its tables (normalizer tries, piece trie, word memo, decode tables --
 * not the per-call workspaces, which grow with the batches a handle sees and are kept: up to SPMX_STREAM_SCRATCH_MB, default
 * 16 GB, for the streaming kernels' text columns) and the wall-clock milliseconds of spmx_create: parse + table build + upload.
 * No reference counterpart (the reference's Load builds its tries on the host, sentencepiece_processor.cc:231-275); either
 * pointer may be null. */
int spmx_handle_info(const spmx_handle *h, uint64_t *table_bytes, double *load_ms);

#ifdef __cplusplus
}
#endif
#endif
