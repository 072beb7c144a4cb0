/* ngram_search.h — C ABI of libngram_search.so, the MI355X-native n-gram fuzzy search engine.
 *
 * Drop-in boundary: the first eight entry points have exactly the signatures, argument
 * meaning, ownership rules and error behaviour of the reference DLL's exports
 * (serena-yu17/StringSearchLib, nGramSearch/dllmain.cpp; line numbers below). A host that
 * binds the reference through its C ABI binds this library unchanged.
 *
 * The search path runs on the GPU: queries are normalised, hashed into 3-grams, matched
 * against gram -> term posting lists kept as CSR in HBM, counted in a u4 count-sketch in LDS
 * (candidates resolved exactly; exact LDS hash counting where the sketch cannot decide),
 * weighted, merged per key and cut to `limit` by HIP kernels for gfx950. indexN interns the
 * strings and builds the CSR on the GPU (ngs_intern.hip, ngs_build.hip; for gram dictionaries of
 * other gram sizes the GPU also finds the distinct gram keys and the host lays out only their
 * lookup table) and keeps it resident. There is no CPU search fallback: if no
 * GPU is usable, indexN prints the HIP error and returns 0.
 *
 * Threading: one global reader/writer lock, as the reference (dllmain.cpp:22). indexN and
 * dispose are exclusive; everything else may run concurrently (each call takes its own
 * stream and scratch from the handle's pool).
 */
#ifndef NGRAM_SEARCH_H
#define NGRAM_SEARCH_H

#include <stddef.h>
#include <stdint.h>
#include <wchar.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NGS_API __attribute__((visibility("default")))

/* ------------------------------------------------------------------------------------
 * Reference exports (nGramSearch/dllmain.cpp), identical signatures.
 * ------------------------------------------------------------------------------------ */

/* dllmain.cpp:37. Index `size` words laid out as rows of `rowSize` (first word of a row =
 * master key, the rest aliases). `weight` (may be NULL) is indexed by FLAT word index;
 * weight 0 drops the pair. Returns the smallest free handle >= 1; 0 on failure. A
 * library with size < 2 or words == NULL yields a handle whose searches return 0. */
NGS_API uint32_t indexN(char** words, uint64_t size, uint16_t rowSize, float* weight);

/* dllmain.cpp:61. Like score() without the scores array. */
NGS_API uint32_t search(uint32_t handle, const char* query, char*** results, float threshold,
                        uint32_t limit);

/* dllmain.cpp:82. Top-`limit` master keys for `query` (limit 0 = unlimited) whose match
 * ratio passes `threshold`, sorted by score desc then key length asc. *results receives a
 * new[]'d array of pointers to index-owned key strings (valid until dispose), *scores a
 * new[]'d float array; free both with release(). Returns the count. Unknown handle or
 * un-built index: returns 0 and leaves *results / *scores untouched. */
NGS_API uint32_t score(uint32_t handle, const char* query, char*** results, float** scores,
                       float threshold, uint32_t limit);

/* dllmain.cpp:98. delete[]s arrays returned by search/score/searchBatch/scoreBatch. Either may be
 * NULL; scoreBatchSim's third array goes through the float argument: release(handle, NULL, sims). */
NGS_API void release(uint32_t handle, char** results, float* scores);

/* dllmain.cpp:110. Frees the index (host and device). Unknown handles are ignored. */
NGS_API void dispose(uint32_t handle);

/* dllmain.cpp:120. Number of distinct normalised terms (wordMap.size()). */
NGS_API uint64_t getSize(uint32_t handle);

/* dllmain.cpp:133. Number of distinct 3-grams over the long terms (ngrams.size()). */
NGS_API uint64_t getLibSize(uint32_t handle);

/* dllmain.cpp:142. Replaces the set of bytes kept by query normalisation (others become
 * spaces) for later searches. The index itself keeps the default set it was built with. */
NGS_API void setValidChar(uint32_t handle, char* characters, int n);

/* ------------------------------------------------------------------------------------
 * Batch extensions (BASELINE.json north_star: "the batched search() scoring loop").
 * Same semantics as score()/search() for each query; one GPU pass for the whole batch.
 * counts[i] = results of query i; *results / *scores are ONE flat new[]'d array each,
 * query i's results starting at sum(counts[0..i)). Returns the total; free with release().
 * Unknown handle / un-built index: returns 0, counts zeroed, outputs untouched.
 * ------------------------------------------------------------------------------------ */
NGS_API uint32_t scoreBatch(uint32_t handle, const char* const* queries, uint32_t nQueries,
                            float threshold, uint32_t limit, uint32_t* counts, char*** results,
                            float** scores);
NGS_API uint32_t searchBatch(uint32_t handle, const char* const* queries, uint32_t nQueries,
                             float threshold, uint32_t limit, uint32_t* counts, char*** results);

/* ------------------------------------------------------------------------------------
 * Gram-size and wide-string extensions (BASELINE config 4; Readme.md:47,91,135,170,190,208
 * documents indexW/searchW/releaseW/disposeW/getSizeW/getLibSizeW with a gSize parameter,
 * but the reference code has neither — parity self-consistent only).
 * Handles are shared with the narrow API; wchar_t is 4 bytes (UTF-32) on Linux.
 * Every threshold of the reference scales with g: terms of length >= 2g are gram-indexed,
 * queries shorter than 3g also run the edit-distance search, queries of <= g characters
 * scan the whole library, a query of m characters has m - g + 1 grams.
 * Wide normalisation: code points < 128 follow the byte rules (validChar, toupper);
 * code points >= 128 are kept as they are; values > 0x10FFFF become spaces.
 * ------------------------------------------------------------------------------------ */

/* indexN with grams of gSize (1..3) bytes; gSize 3 is indexN. Returns 0 for other gSize. */
NGS_API uint32_t indexG(char** words, uint64_t size, uint16_t rowSize, float* weight, uint16_t gSize);
/* Wide index (Readme.md:91): words are NUL-terminated UTF-32 strings; gSize 1..3. */
NGS_API uint32_t indexW(wchar_t** words, uint64_t size, uint16_t rowSize, float* weight, uint16_t gSize);
/* Wide search/score (Readme.md:135) on an indexW handle; result strings are index-owned
 * wchar_t keys. Return 0 on a narrow handle (and the narrow calls return 0 on a wide one). */
NGS_API uint32_t searchW(uint32_t handle, const wchar_t* query, wchar_t*** results, float threshold,
                         uint32_t limit);
NGS_API uint32_t scoreW(uint32_t handle, const wchar_t* query, wchar_t*** results, float** scores,
                        float threshold, uint32_t limit);
NGS_API uint32_t scoreBatchW(uint32_t handle, const wchar_t* const* queries, uint32_t nQueries,
                             float threshold, uint32_t limit, uint32_t* counts, wchar_t*** results,
                             float** scores);
NGS_API uint32_t searchBatchW(uint32_t handle, const wchar_t* const* queries, uint32_t nQueries,
                              float threshold, uint32_t limit, uint32_t* counts, wchar_t*** results);
/* Readme.md:170,190,208,226 — same meaning as release/dispose/getSize/getLibSize. */
NGS_API void releaseW(uint32_t handle, wchar_t** results, float* scores);
NGS_API void disposeW(uint32_t handle);
NGS_API uint64_t getSizeW(uint32_t handle);
NGS_API uint64_t getLibSizeW(uint32_t handle);

/* ------------------------------------------------------------------------------------
 * UTF-8 on wide indexes. Linux hosts hold UTF-8 (files, databases, Arrow and torch byte
 * buffers, char*), not wchar_t: these entry points take and return UTF-8 and run the wide
 * index and search underneath. They are valid on any wide handle (indexW, indexU8, or a wide
 * index loaded from a file); on a narrow handle they answer like the width mismatch above
 * (0 / NULL / -3). The W calls and the device entry points work on an indexU8 handle too.
 * Decoding rule: where a well-formed UTF-8 sequence (the Unicode standard's table: no overlong
 * forms, no surrogates, at most U+10FFFF) starts and lies inside the string, it is one character,
 * its scalar value; any other byte b is one unit 0x110000 + b, which is not a code point and is
 * normalised to a space like an invalid byte of the narrow API. (Python: bytes.decode('utf-8',
 * 'surrogateescape') with U+DC80+x read as 0x110000 + 0x80 + x.) Encoding inverts it exactly, so
 * result strings are the bytes that were indexed.
 * ------------------------------------------------------------------------------------ */

/* indexW over UTF-8 words (decoded on the host): gSize 1..3, 0 otherwise; size < 2 or
 * words == NULL yields an un-built wide handle, as indexW. */
NGS_API uint32_t indexU8(char** words, uint64_t size, uint16_t rowSize, float* weight, uint16_t gSize);
/* search / score / searchBatch / scoreBatch with UTF-8 queries: the answers (keys, order, fp32
 * scores, counts) are those of the W call on the decoded queries. Result strings are index-owned
 * NUL-terminated UTF-8 keys (valid until dispose; the table of them is built by the first U8 call
 * on the handle); free the arrays with release(). Batches of more than 16 queries are uploaded as
 * UTF-8 and decoded on the GPU. On a handle with several replicas a U8 batch is answered by the
 * first replica, not split (the results are identical). */
NGS_API uint32_t searchU8(uint32_t handle, const char* query, char*** results, float threshold, uint32_t limit);
NGS_API uint32_t scoreU8(uint32_t handle, const char* query, char*** results, float** scores, float threshold,
                         uint32_t limit);
NGS_API uint32_t scoreBatchU8(uint32_t handle, const char* const* queries, uint32_t nQueries, float threshold,
                              uint32_t limit, uint32_t* counts, char*** results, float** scores);
NGS_API uint32_t searchBatchU8(uint32_t handle, const char* const* queries, uint32_t nQueries, float threshold,
                               uint32_t limit, uint32_t* counts, char*** results);
/* UTF-8 form of ngsKeyW (NULL if out of range, un-built, or a narrow index). A key character an
 * indexW caller stored that is neither a scalar value nor 0x110000 + b reads as U+FFFD. */
NGS_API const char* ngsKeyU8(uint32_t handle, uint32_t keyId);

/* ------------------------------------------------------------------------------------
 * Device-level extensions: inputs and outputs stay in HBM (bench, multi-GPU sharding,
 * host frameworks that already hold device buffers). Not in the reference.
 * ------------------------------------------------------------------------------------ */

/* Selects the HIP device that the calling thread's next indexN builds on (default: the
 * current HIP device). Same as ngsSetDevices(&device, 1). Returns 0, or a negative HIP error code. */
NGS_API int ngsSetDevice(int device);
/* Multi-GPU (BASELINE north_star: "one-shard-per-GPU across the node"): the calling thread's next
 * indexN / indexG / indexW places one replica of the index on each of the n devices (repeats
 * allowed; n = 0 restores the default). score/search/scoreBatch/searchBatch on such a handle
 * split a batch of at least 4,096 queries per replica into contiguous slices, one per replica,
 * scored concurrently (one host thread and stream each) and joined in query order: the results
 * are those of one device. ngsSearchDevice uses the replica on the caller's current device
 * (-3 if the index has none there).
 * Returns 0, or a negative HIP error code (nothing changed). */
NGS_API int ngsSetDevices(const int* devices, int n);
/* Replicas of the index (devices it was placed on); -1 for an unknown handle. */
NGS_API int ngsReplicaCount(uint32_t handle);
NGS_API int ngsDeviceCount(void);

/* Number of master keys; key ids used by ngsSearchDevice are 0..n-1. */
NGS_API uint32_t ngsNumKeys(uint32_t handle);
/* NUL-terminated, index-owned string of key `keyId` (NULL if out of range or if the
 * index's character width differs: ngsKey for narrow indexes, ngsKeyW for indexW). */
NGS_API const char* ngsKey(uint32_t handle, uint32_t keyId);
NGS_API const wchar_t* ngsKeyW(uint32_t handle, uint32_t keyId);
/* Character width in bytes (1 or 4) and gram size of the index; 0 for an unknown handle. */
NGS_API uint32_t ngsCharSize(uint32_t handle);
NGS_API uint32_t ngsGramSize(uint32_t handle);

/* Scores nQueries queries held on the handle's device: query i is the raw bytes
 * dQueryBytes[dQueryOffsets[i] .. dQueryOffsets[i+1]) (no NUL needed; for an indexW handle
 * the bytes are UTF-32 characters and the offsets multiples of 4). Writes, for query i,
 * dCounts[i] results to dKeys/dScores[i*outStride ...]; outStride must be >=
 * min(limit ? limit : 2^31-1, ngsNumKeys). `stream` is the caller's hipStream_t (NULL = the
 * null stream): the call's kernels are ordered after the work already queued on it, and the
 * call returns when the results are complete.
 * Returns 0, or a negative error (-1 bad handle, -2 un-built index, -3 bad argument,
 * -4 HIP failure, -5 internal error flagged by a kernel, e.g. an exhausted LDS table). */
NGS_API int ngsSearchDevice(uint32_t handle, const uint8_t* dQueryBytes, const uint64_t* dQueryOffsets,
                            uint32_t nQueries, float threshold, uint32_t limit, uint32_t outStride,
                            uint32_t* dCounts, uint32_t* dKeys, float* dScores, void* stream);

/* Asynchronous ngsSearchDevice: the call is ordered after the work already queued on `stream`,
 * runs on streams of its own and returns once it is queued, with a ticket. The results are
 * complete when ngsSearchDeviceWait(handle, ticket) returns 0 (it waits, runs the library-wide
 * path for the rare queries that need it and records the statistics); every ticket must be
 * waited for once, and the output buffers must not be read or reused before. Calls in flight
 * together overlap on the GPU (a batch's tail beside the next batch's counting). Return codes
 * as ngsSearchDevice; Wait answers -3 for an unknown ticket. dispose() waits for calls in flight. */
NGS_API int ngsSearchDeviceAsync(uint32_t handle, const uint8_t* dQueryBytes, const uint64_t* dQueryOffsets,
                                 uint32_t nQueries, float threshold, uint32_t limit, uint32_t outStride,
                                 uint32_t* dCounts, uint32_t* dKeys, float* dScores, void* stream,
                                 uint64_t* ticket);
NGS_API int ngsSearchDeviceWait(uint32_t handle, uint64_t ticket);

/* Decodes a batch of UTF-8 strings held on the current device into the UTF-32 batch that
 * ngsSearchDevice / ngsSearchDeviceAsync take for a wide index: string i is the bytes
 * dBytes[dOffsets[i] .. dOffsets[i+1]) (absolute offsets, any alignment, dOffsets[0] need not be
 * 0); its characters go to dOut (4-byte aligned) from byte dOutOffsets[i], and dOutOffsets[0..n]
 * ascend from 0 in multiples of 4. A string whose characters would end past outCapBytes is decoded
 * as empty, like every string after it, and nothing of it is written; outCapBytes = 4 x the input
 * byte count always suffices. Stream-ordered on `stream` with no host wait and no handle: queued
 * before ngsSearchDevice / ngsSearchDeviceAsync on the same stream, it gives a caller with UTF-8
 * in HBM the whole asynchronous path. Returns 0, -3 (bad argument), -4 (HIP error). */
NGS_API int ngsUtf8Decode(const uint8_t* dBytes, const uint64_t* dOffsets, uint32_t n, uint8_t* dOut,
                          uint64_t outCapBytes, uint64_t* dOutOffsets, void* stream);
/* ngsSearchDevice with UTF-8 queries on a wide handle (-3 on a narrow one): the synchronous
 * convenience form, decoding into the call's own scratch first. Return codes as ngsSearchDevice. */
NGS_API int ngsSearchDeviceU8(uint32_t handle, const uint8_t* dQueryBytes, const uint64_t* dQueryOffsets,
                              uint32_t nQueries, float threshold, uint32_t limit, uint32_t outStride,
                              uint32_t* dCounts, uint32_t* dKeys, float* dScores, void* stream);

/* Low-latency score()/search() (narrow indexes): a persistent one-wave server kernel answers
 * single queries from a request block in pinned host memory, with no kernel launch, copy or
 * stream wait per call. It serves libraries small enough that one wave searches a query (fewer
 * than 16 skip buckets; large libraries keep the sliced latency path) and limits up to 128; other
 * calls take the regular path. It starts by itself on such a library after the 4th score()/
 * search() call; ngsServe(h, 1) starts it at once, ngsServe(h, 0) stops it and turns the automatic
 * start off. The kernel leaves after 200 ms without a request (or 10 s of life) and is relaunched
 * on the next call; a batch call (scoreBatch/searchBatch of more than 16 queries, the device entry
 * points) stops it first and keeps it stopped until the batch is done, so no batch kernel queues
 * behind it; dispose() stops it. Answers are the regular path's, bit for bit. One request at a
 * time per handle: a call that finds the server busy takes the regular path. Returns 0, -1 (bad
 * handle), -2 (unbuilt index), -3 (wide index), -4 (HIP error). */
NGS_API int ngsServe(uint32_t handle, int enable);
/* Packs a device result block in ngsSearchDevice's layout (counts[n], query i's records at
 * i * stride) on `stream`: dOffsets[n + 1] = exclusive prefix sum of the counts (dOffsets[n] = total
 * records) and dRecords[2 * total] = {key id, fp32 score bits} per record in query order. Used by the
 * multi-GPU gather (stringsearchlib_amd/shard.py) so that the bytes sent to rank 0 follow the
 * results, not n x stride. The block may come from anywhere: a count above `stride` is read as
 * `stride`, by the prefix sum as by the copy (as ngsSimilarityDevice reads it), so dOffsets[n] is
 * always the number of records written. The offsets are 32-bit: n x stride > 0xFFFFFFFF is refused
 * with -3 before anything is queued or read. Returns 0, -3 (bad argument: NULL dCounts or dOffsets;
 * with n > 0, stride 0 or NULL dKeys, dScores or dRecords; the overflow above), -4 (HIP error). */
NGS_API int ngsPackResults(const uint32_t* dCounts, const uint32_t* dKeys, const float* dScores, uint32_t n,
                           uint32_t stride, uint32_t* dOffsets, uint32_t* dRecords, void* stream);

/* ------------------------------------------------------------------------------------
 * Edit-distance similarity and re-ranking of a result block on the device (not in the
 * reference). The search's score (weight x shared grams / query grams) is a candidate filter;
 * these stages verify the candidates where they lie, in HBM, as stream-ordered stages behind
 * ngsSearchDevice / ngsSearchDeviceAsync (after its Wait) on the caller's stream.
 *
 * The similarity of a record (query i, key k):
 *   Q  = the query normalised as the search does it: every character through escapeBlank with the
 *        handle's validChar set at the time of the call, blanks trimmed at both ends, toupper;
 *        m = |Q| in characters (bytes; UTF-32 units on a wide index);
 *   T  = a normalised term of the index (built with the default set, L = |T| >= 1); the terms of
 *        key k are those of every (term, key) pair the index holds, whatever the weight;
 *   d  = the unit-cost Levenshtein distance of Q and T (insert, delete, substitute; global);
 *   sim(Q, T) = 1.0f - (float)d / (float)max(m, L), in fp32 (one correctly rounded division, one
 *        subtraction: numpy.float32 arithmetic gives the same bits);
 *   sim(record) = the largest sim(Q, T) over the terms T of key k: a query that matched an alias
 *        gets the alias's similarity, not the master string's.
 * A wildcard query (raw length 0, or the single character '*') has sim 1.0f on every record,
 * whatever its key id. Otherwise a query of more than 4,096 normalised characters, or a key id
 * >= ngsNumKeys, has sim -1.0f ("not computed"; nothing is read through the id), which filters and
 * orders like any other value. A count above `stride` is read as `stride`.
 * The query bytes and offsets have exactly ngsSearchDevice's layout: pass the same buffers (for a
 * wide handle UTF-32 units and offsets in multiples of 4, e.g. those ngsUtf8Decode wrote).
 * Both calls use the replica on the caller's current device, queue their kernels on `stream` and
 * return without waiting. (On an index whose keys have one pair each, the first call on a replica
 * builds a 4-byte-per-key map on the device and waits for that once.) Arguments are checked before
 * anything else: -3 bad argument, then -1 bad handle, -2 un-built index, -3 no replica on the
 * current device, -4 HIP error.
 * ------------------------------------------------------------------------------------ */

/* dSim[i*stride + r] for r < dCounts[i]: the similarity above of query i and key dKeys[i*stride + r].
 * Reads dCounts/dKeys, writes only dSim. Stream-ordered on `stream`, no host wait.
 * 0, -1 bad handle, -2 un-built, -3 bad argument / no replica on the current device, -4 HIP error. */
NGS_API int ngsSimilarityDevice(uint32_t handle, const uint8_t* dQueryBytes, const uint64_t* dQueryOffsets,
                                uint32_t nQueries, uint32_t stride, const uint32_t* dCounts,
                                const uint32_t* dKeys, float* dSim, void* stream);

/* ngsSimilarityDevice, then per query: records with sim < minSimilarity are dropped, the rest put in
 * order of (sim descending, previous position ascending). dCounts, dKeys, dScores and dSim are
 * rewritten in place (entries past the new count are unspecified). stride <= kRerankMaxStride (4,096),
 * minSimilarity not NaN, else -3. Stream-ordered, no host wait. */
NGS_API int ngsRerankDevice(uint32_t handle, const uint8_t* dQueryBytes, const uint64_t* dQueryOffsets,
                            uint32_t nQueries, uint32_t stride, uint32_t* dCounts, uint32_t* dKeys,
                            float* dScores, float* dSim, float minSimilarity, void* stream);

/* scoreBatch / scoreBatchW / scoreBatchU8 followed by the re-rank: query i's counts[i] results are
 * those of the search that pass minSimilarity, in order of (sim descending, the search's order
 * ascending); *sims is a third flat new[]'d array beside *results and *scores, sims[j] belonging to
 * results[j]. Free it with release(handle, NULL, sims) (release delete[]s a float array), the other
 * two as usual. The effective limit min(limit or 2^31-1, ngsNumKeys) must not exceed 4,096: above it
 * the call fails (returns 0, counts zeroed, outputs untouched) and ngsLastError() is
 * NGS_ERR_RERANK_LIMIT. Unknown handle, un-built index, width mismatch, NaN minSimilarity: 0, counts
 * zeroed, outputs untouched. The first replica answers. */
NGS_API uint32_t scoreBatchSim(uint32_t handle, const char* const* queries, uint32_t nQueries, float threshold,
                               uint32_t limit, float minSimilarity, uint32_t* counts, char*** results,
                               float** scores, float** sims);
NGS_API uint32_t scoreBatchSimW(uint32_t handle, const wchar_t* const* queries, uint32_t nQueries, float threshold,
                                uint32_t limit, float minSimilarity, uint32_t* counts, wchar_t*** results,
                                float** scores, float** sims);
NGS_API uint32_t scoreBatchSimU8(uint32_t handle, const char* const* queries, uint32_t nQueries, float threshold,
                                 uint32_t limit, float minSimilarity, uint32_t* counts, char*** results,
                                 float** scores, float** sims);

/* ------------------------------------------------------------------------------------
 * Self-join on the device: the near-duplicates of the library's own keys and their clusters (not
 * in the reference). The key strings already lie in HBM, so "the library against itself" is a
 * pipeline of stream-ordered stages in front of and behind ngsSearchDevice: the keys written as a
 * query batch, the search, the key's own record removed, connected components over the (key, key)
 * records that remain. Nothing goes through the host in between.
 *
 * The device entry points use the replica on the caller's current device and queue on `stream`.
 * Arguments are checked before anything else: -3 bad argument (NULL pointers), then -1 bad handle,
 * -2 un-built index, -3 a key range past ngsNumKeys, a capacity or stride too small, or no replica on
 * the current device, -4 HIP error. ngsDropSelfDevice and ngsClusterDevice take no handle.
 * ------------------------------------------------------------------------------------ */

/* The bytes the keys [firstKey, firstKey + nKeys) occupy as a query batch: their characters without
 * the NULs, times the character width. 0 for a bad handle, an un-built index or a range past
 * ngsNumKeys (and for nKeys = 0). */
NGS_API uint64_t ngsKeyQueryBytes(uint32_t handle, uint32_t firstKey, uint32_t nKeys);

/* Writes those keys in ngsSearchDevice's query layout: query i is key firstKey + i as ngsKey / ngsKeyW
 * returns it, without its NUL, at dBytes[dOffsets[i] .. dOffsets[i+1]); dOffsets[0..nKeys] ascend from 0
 * (on a wide index the units are UTF-32, the offsets multiples of 4 and dBytes must be 4-byte aligned).
 * Nothing past dBytes[ngsKeyQueryBytes(...)] is written. capBytes below ngsKeyQueryBytes(...) or a range
 * past the keys: -3. nKeys = 0 is valid (firstKey up to ngsNumKeys), writes dOffsets[0] = 0 only and
 * reads nothing of the index but the offset entry of firstKey. Stream-ordered, no host wait. */
NGS_API int ngsKeyQueriesDevice(uint32_t handle, uint32_t firstKey, uint32_t nKeys, uint8_t* dBytes,
                                uint64_t capBytes, uint64_t* dOffsets, void* stream);

/* Per row i < n of a result block (ngsSearchDevice's layout), in place: the record whose key id is
 * firstKey + i is removed if there is one (at most one exists, wherever it stands) and the records
 * behind it move up by one; the row is cut to `limit` records (0: no cut); dCounts[i] is the new count.
 * A count above `stride` is read as `stride`. Cells past the new count are unspecified; nothing beyond
 * i * stride + stride is written. Stream-ordered, no host wait. 0, -3 (NULL dCounts; NULL dKeys or
 * dScores with n and stride non-zero), -4 HIP error. */
NGS_API int ngsDropSelfDevice(uint32_t* dCounts, uint32_t* dKeys, float* dScores, uint32_t n, uint32_t stride,
                              uint32_t firstKey, uint32_t limit, void* stream);

/* The join of keys [firstKey, firstKey + nKeys): row i (dCounts[i], records at i * outStride) is the
 * answer ngsSearchDevice gives for the string of key firstKey + i over the library without that key:
 * the full ranking at `threshold` with the key's own record removed, then the first `limit` (0: all).
 * That is the search with limit + 1 and the key's own record dropped, whether or not it is among the
 * hits (a key need not find itself: a zero or negative weight, a string the validChar set blanks).
 * It runs ngsKeyQueriesDevice into the call's own scratch, ngsSearchDevice with that limit into the
 * caller's block and ngsDropSelfDevice. outStride must be at least
 * min((limit ? limit : 2^31-1) + 1, ngsNumKeys), one more than the search of the same limit asks, for
 * the record that is found and removed: anything less is -3. The queries are normalised with the
 * handle's current validChar set, like any query. Returns when the results are complete; return codes
 * as ngsSearchDevice. */
NGS_API int ngsSelfJoinDevice(uint32_t handle, uint32_t firstKey, uint32_t nKeys, float threshold, uint32_t limit,
                              uint32_t outStride, uint32_t* dCounts, uint32_t* dKeys, float* dScores, void* stream);

/* Connected components. The block is read as undirected edges (firstKey + i, dKeys[i * stride + r]),
 * r < min(dCounts[i], stride); an edge with an end >= nLabels is ignored and nothing is read through
 * that id. NGS_CLUSTER_INIT first sets dLabels[k] = k for k < nLabels; NGS_CLUSTER_FINISH afterwards
 * makes dLabels[k] the smallest id of k's component. Without FINISH dLabels is a forest with
 * dLabels[k] <= k that later calls merge further blocks into; n = 0 with a flag is valid (init only,
 * finish only). The result does not depend on the order the edges arrive in: it is exactly
 * reproducible. Stream-ordered, no host wait. 0, -3 (an unknown flag, NULL dLabels with nLabels, NULL
 * dCounts or dKeys with n and stride non-zero), -4 HIP error. */
#define NGS_CLUSTER_INIT 1u
#define NGS_CLUSTER_FINISH 2u
NGS_API int ngsClusterDevice(const uint32_t* dCounts, const uint32_t* dKeys, uint32_t n, uint32_t stride,
                             uint32_t firstKey, uint32_t* dLabels, uint32_t nLabels, uint32_t flags, void* stream);

/* The join of keys [firstKey, firstKey + nKeys) into caller-allocated arrays: counts[nKeys], row i's
 * records (key ids, scores) at i * stride, stride >= min(limit ? limit : 2^31-1, ngsNumKeys). Runs on
 * the first replica in batches of at most 65,536 keys and returns the total number of records. On
 * failure (unknown handle, un-built index, range past the keys, stride too small, HIP error) it returns
 * 0, zeroes the counts and sets ngsLastError. */
NGS_API uint32_t selfJoin(uint32_t handle, uint32_t firstKey, uint32_t nKeys, float threshold, uint32_t limit,
                          uint32_t stride, uint32_t* counts, uint32_t* keyIds, float* scores);

/* Clusters of near-duplicate keys: labels[ngsNumKeys] (caller-allocated), labels[k] = the smallest key
 * id of k's cluster. The edges are the records of the self-join at (threshold, limit), limit in
 * 1..4,096; with minSimilarity > -1.0f only those whose edit-distance similarity (above: the key's
 * string as the query) is at least minSimilarity. batchKeys: keys per batch (0 = 65,536); the label
 * array stays on the device across the batches and is finished and read back once. The filter keeps
 * a record unless its similarity is below minSimilarity, in the search's order; it is not
 * ngsRerankDevice (no sort, no cap on the stride). What the similarity's special values mean for it:
 * a key of more than 4,096 normalised characters has -1.0f ("not computed") on all of its own row's
 * records, so with a filter it gives no edge (other keys' rows may still link to it); the key "*" is a
 * wildcard query with similarity 1.0f on every record, so its row keeps all of them; the similarity
 * is never NaN (a NaN would be kept). Returns the number
 * of clusters; 0 with ngsLastError set when the limit is 0 (a HIP invalid-value code) or above 4,096
 * (NGS_ERR_RERANK_LIMIT), minSimilarity is NaN, the handle is unknown or un-built, or HIP fails. */
NGS_API uint32_t dedupKeys(uint32_t handle, float threshold, uint32_t limit, float minSimilarity,
                           uint32_t batchKeys, uint32_t* labels);

/* ------------------------------------------------------------------------------------
 * The similarity by a metric, and the term that matched (not in the reference). Q (length m), T
 * (length L >= 1), the wildcard rule, the cap of 4,096 normalised characters, "a count above the
 * stride reads as the stride" and "key id >= ngsNumKeys is -1.0f" are exactly those of the
 * edit-distance similarity above. The metric selects d and the divisor:
 *   NGS_SIM_LEVENSHTEIN  d = Levenshtein, sim = 1.0f - (float)d / (float)max(m, L): the bits of the
 *                        entry points without a metric;
 *   NGS_SIM_OSA          optimal string alignment: Levenshtein plus the swap of two adjacent
 *                        characters at cost 1, no substring edited twice:
 *                        D[i][j] = min(D[i-1][j] + 1, D[i][j-1] + 1, D[i-1][j-1] + [Q_i != T_j],
 *                                      D[i-2][j-2] + 1 if Q_i = T_{j-1} and Q_{i-1} = T_j);
 *                        sim = 1.0f - (float)d / (float)max(m, L); an empty Q has d = L, sim 0.0f;
 *   NGS_SIM_PARTIAL      d = the least Levenshtein(Q, T[a..b)) over 0 <= a <= b <= L (both ends of T
 *                        free, the empty substring allowed, so d <= m);
 *                        sim = 1.0f - (float)d / (float)m for m >= 1, 0.0f for m = 0. It is directional:
 *                        Q inside T scores 1.0f, T inside Q does not.
 * Each is one correctly rounded fp32 division and one subtraction. A record's similarity is the
 * largest over the key's non-empty terms. The matched term is the term id (0 .. getSize - 1, see
 * ngsTerm) that attains it, the smallest id among several of the same fp32 value, and 0xFFFFFFFF
 * where no term was compared: wildcard rows, -1.0f rows, a key without a non-empty term.
 * An unknown metric is a bad argument (-3), checked with the other arguments before the handle.
 * ------------------------------------------------------------------------------------ */
#define NGS_SIM_LEVENSHTEIN 0u
#define NGS_SIM_OSA 1u
#define NGS_SIM_PARTIAL 2u

/* ngsSimilarityDevice by `metric`; dTerms (may be NULL: not wanted, and then nothing is spent on it)
 * receives the matched term ids in dSim's layout. Return codes as ngsSimilarityDevice. */
NGS_API int ngsSimilarityDeviceM(uint32_t handle, const uint8_t* dQueryBytes, const uint64_t* dQueryOffsets,
                                 uint32_t nQueries, uint32_t stride, const uint32_t* dCounts,
                                 const uint32_t* dKeys, uint32_t metric, float* dSim, uint32_t* dTerms,
                                 void* stream);

/* ngsRerankDevice by `metric`; dTerms (may be NULL) is filled and permuted in place with dKeys,
 * dScores and dSim. Return codes as ngsRerankDevice. */
NGS_API int ngsRerankDeviceM(uint32_t handle, const uint8_t* dQueryBytes, const uint64_t* dQueryOffsets,
                             uint32_t nQueries, uint32_t stride, uint32_t* dCounts, uint32_t* dKeys,
                             float* dScores, float* dSim, uint32_t* dTerms, uint32_t metric,
                             float minSimilarity, void* stream);

/* scoreBatchSim / scoreBatchSimW / scoreBatchSimU8 by `metric`. With terms != NULL, *terms is a fourth
 * flat new[]'d array, terms[j] the matched term id of results[j]: free it with ngsReleaseTerms. An
 * unknown metric fails like a NaN minSimilarity: 0, counts zeroed, outputs untouched, ngsLastError a
 * HIP invalid-value code. Everything else as scoreBatchSim. */
NGS_API uint32_t scoreBatchSimM(uint32_t handle, const char* const* queries, uint32_t nQueries, float threshold,
                                uint32_t limit, uint32_t metric, float minSimilarity, uint32_t* counts,
                                char*** results, float** scores, float** sims, uint32_t** terms);
NGS_API uint32_t scoreBatchSimMW(uint32_t handle, const wchar_t* const* queries, uint32_t nQueries, float threshold,
                                 uint32_t limit, uint32_t metric, float minSimilarity, uint32_t* counts,
                                 wchar_t*** results, float** scores, float** sims, uint32_t** terms);
NGS_API uint32_t scoreBatchSimMU8(uint32_t handle, const char* const* queries, uint32_t nQueries, float threshold,
                                  uint32_t limit, uint32_t metric, float minSimilarity, uint32_t* counts,
                                  char*** results, float** scores, float** sims, uint32_t** terms);
/* delete[]s the fourth array of scoreBatchSimM*; NULL is allowed. */
NGS_API void ngsReleaseTerms(uint32_t* terms);

/* dedupKeys with the filter's similarity by `metric` (an unknown one: 0 and a HIP invalid-value code).
 * The special values are handled as dedupKeys documents. NGS_SIM_PARTIAL is directional: the row of
 * key a measures a's string inside key b's terms, the row of b the reverse, and an edge is made if
 * either row keeps its record, as for any record. */
NGS_API uint32_t dedupKeysM(uint32_t handle, float threshold, uint32_t limit, uint32_t metric, float minSimilarity,
                            uint32_t batchKeys, uint32_t* labels);

/* The normalised term `termId` (0 .. getSize(handle) - 1) as the index holds it: bytes on a narrow
 * index, UTF-32 units on a wide one, no terminator. Returns its length in characters whatever capBytes
 * is (size a buffer with buf = NULL, capBytes = 0) and copies min(capBytes, length x width) bytes,
 * rounded down to whole characters, into buf. The terms live in device memory only: every call is one
 * small synchronous copy from the first replica, a diagnostic-rate call for showing results, not for
 * bulk export. -1 bad handle, -2 un-built index, -3 id out of range (or NULL buf with a capacity),
 * -4 HIP error. */
NGS_API int64_t ngsTerm(uint32_t handle, uint32_t termId, void* buf, uint64_t capBytes);

/* ------------------------------------------------------------------------------------
 * Token sort: a similarity that does not depend on the order of the words (not in the reference).
 * NGS_SIM_TOKEN_SORT is OR'ed onto one of the three metrics above (a metric is valid iff
 * (metric & ~NGS_SIM_TOKEN_SORT) <= 2; anything else is unknown as before). A record's similarity
 * is then the base metric's sim(Q', T') with the divisor from m' = |Q'| and L' = |T'|, the largest
 * over the key's non-empty terms; the matched term is the ordinary term id; wildcard rows, -1.0f
 * rows and everything else are as above. ngsTerm still returns the term as indexed.
 *
 * The token-sorted form of a string: split it at its separators into tokens (the maximal runs of
 * the other characters), order the tokens by their normalised characters (unsigned values,
 * lexicographically, a proper prefix first, equal tokens in their order of appearance), join them
 * with single blanks. For a query a separator is a character that is blank after the validChar
 * escape, and the characters written are the raw ones; for a term T as the index stores it a
 * separator is a blank, and L' <= L. A string of more than 4,096 characters between its first and
 * last token character stays as it is (the similarity answers -1.0f for such a query), and so does
 * the query "*", which is a wildcard whether or not the validChar set keeps '*'.
 *
 * scoreBatchSimM / MW / MU8 and dedupKeysM sort their queries themselves. The two device entry
 * points, ngsSimilarityDeviceM and ngsRerankDeviceM, do NOT: with the flag they read the
 * token-sorted terms and take the query bytes as given, because they must not wait for the host
 * and the host does not know the batch's byte count. Queue ngsTokenSortDevice on the same stream in
 * front of them (as ngsUtf8Decode goes in front of ngsSearchDevice), behind the search, which needs
 * the queries as they were. The first flagged call on a device builds the sorted terms of the
 * index's copy there, once, synchronously (about the size of the terms themselves).
 * ------------------------------------------------------------------------------------ */
#define NGS_SIM_TOKEN_SORT 0x100u

/* Token-sorts a query batch in ngsSearchDevice's layout: string i, dBytes[dOffsets[i] .. dOffsets[i+1])
 * (bytes on a narrow handle, UTF-32 units at offsets in multiples of 4 on a wide one), is written to
 * dOut at the same offsets: the tokens' raw characters in sorted order, one ' ' (0x20) between
 * neighbours, then ' ' up to the string's length. The length is kept, so "" and "*" stay the
 * wildcards they were, "   " stays three blanks and " *" becomes "* " (or two blanks where the validChar
 * set does not keep '*'), which is no wildcard. The
 * handle supplies the character width and the validChar set as of the call. dOut may be dBytes (in
 * place); nothing outside [dOffsets[0], dOffsets[n]) is written. Queued on `stream`; nothing waits.
 * 0 ok (n = 0 included), -3 NULL dOffsets, or NULL dBytes or dOut with n > 0, -1 bad handle,
 * -2 un-built index, -4 HIP error. */
NGS_API int ngsTokenSortDevice(uint32_t handle, const uint8_t* dBytes, const uint64_t* dOffsets, uint32_t n,
                               uint8_t* dOut, void* stream);

/* ------------------------------------------------------------------------------------
 * Linking two indexes: which key of a target index T each key of a source index S corresponds to
 * (not in the reference). nS and nT are their ngsNumKeys.
 *
 * Candidate row. The row of source key a is the answer ngsSearchDevice on T gives at (threshold,
 * limit) for the string of key a of S, as ngsKey / ngsKeyW returns it without its NUL, normalised
 * with T's current validChar set like any query. No record is dropped: S and T may be one handle, and
 * then a key may find itself. limit is 1..4,096 and Ls = min(limit, nT) is the row stride.
 *
 * Similarity filter. With minSimilarity > -1.0f a record is kept unless its similarity is below
 * minSimilarity, in the search's order (dedupKeysM's filter). The similarity is
 * ngsSimilarityDeviceM's on T by `metric`: the query is S's key string, the terms are T's. With
 * NGS_SIM_TOKEN_SORT the batch is token-sorted in place behind the search.
 *
 * Value and edge order. The value of a record is its similarity when the filter is on and its score
 * when it is off. An edge is (a, b, value). Edges are totally ordered by value descending, then a
 * ascending, then b ascending; values compare by the order image of their fp32 bits (bits with the
 * sign bit set inverted, the others with the sign bit set): numeric order for non-NaN floats, with
 * -0 < +0, and a NaN where its bits put it.
 *
 * Modes. NGS_LINK_BEST: match[a] is the b of a's first edge in that order, NGS_NO_MATCH for an empty
 * row; many a may share a b. NGS_LINK_ONE_TO_ONE: the greedy matching: go through all edges in that
 * order and take an edge iff both its ends are still free; match[a] is the b taken for a, or
 * NGS_NO_MATCH. The result is unique: it does not depend on batches, scheduling or replicas.
 *
 * The device composition: ngsKeyQueriesDevice on S, ngsSearchDevice on T (and, for a filter,
 * ngsSimilarityDeviceM on T), then ngsMatchDevice over the block, all on one stream and one device.
 * ------------------------------------------------------------------------------------ */
#define NGS_NO_MATCH 0xFFFFFFFFu

/* The greedy one-to-one matching of a block in rounds. The block has ngsSearchDevice's layout; its
 * edges are (firstKey + i, dKeys[i * stride + r], dValues[i * stride + r]) for r < min(dCounts[i],
 * stride); dValues is the caller's choice, dScores or dSim. An edge with a >= nA or b >= nB is
 * ignored, and nothing is read through that id. dMatchA[nA] and dMatchB[nB] are the matching from
 * both sides (dMatchA[a] = b and dMatchB[b] = a, NGS_NO_MATCH for a free end), dBids[nB] is scratch,
 * *dMatched the number of pairs. The flags of one call run in the order INIT, BEGIN, BID, ACCEPT.
 *
 * An edge is live when both its ends are unmatched. A round is BEGIN, then BID over every block, then
 * ACCEPT over every block: BID makes dBids[b] the largest live edge at b, ACCEPT lets every unmatched
 * row take its own largest live edge if dBids names that same edge, and adds the pairs to *dMatched.
 * A caller with one block passes BEGIN | BID | ACCEPT, plus INIT the first time; a caller with
 * several passes BEGIN | BID on the first block, BID on the others, then ACCEPT on each. A row
 * (a value of firstKey + i) belongs to one block. The matching is complete after the first round
 * that adds nothing to *dMatched: read the word between rounds. Every round with live edges matches
 * at least one pair, a round on a complete matching changes nothing, and the result is exactly the
 * greedy matching above whatever order the rows run in. Stream-ordered, no host wait.
 * 0; -3 an unknown flag, NULL dMatched, NULL dMatchA with nA non-zero, NULL dMatchB or dBids with nB
 * non-zero, NULL dCounts, dKeys or dValues with n and stride non-zero and BID or ACCEPT set; -4 HIP
 * error. n = 0 with flags is valid. */
#define NGS_MATCH_INIT 1u   /* dMatchA[0..nA) = dMatchB[0..nB) = NGS_NO_MATCH, *dMatched = 0 */
#define NGS_MATCH_BEGIN 2u  /* a round starts: the bids are cleared */
#define NGS_MATCH_BID 4u    /* the block's live edges bid for their b */
#define NGS_MATCH_ACCEPT 8u /* the block's rows take the edges that won at both ends */
NGS_API int ngsMatchDevice(const uint32_t* dCounts, const uint32_t* dKeys, const float* dValues, uint32_t n,
                           uint32_t stride, uint32_t firstKey, uint32_t* dMatchA, uint32_t nA, uint32_t* dMatchB,
                           uint32_t nB, uint64_t* dBids, uint32_t* dMatched, uint32_t flags, void* stream);

/* Links the keys of hFrom (S) to the keys of hTo (T) as defined above: match[nS] (caller-allocated),
 * and for the chosen record of each source key scores[nS] and sims[nS] (each may be NULL): 0.0f and
 * -1.0f for an unmatched key, sims all -1.0f when the filter is off (nothing was computed). Returns
 * the number of matched source keys. T's first replica answers, and S must have a replica on that
 * device. batchKeys: source keys per batch (0 = 65,536). NGS_LINK_BEST holds one batch's block on
 * the device; NGS_LINK_ONE_TO_ONE holds the whole block of nS x Ls records (keys, scores, and
 * similarities with a filter: 8 or 12 bytes a record) and runs rounds over it until one adds
 * nothing. Everything is read back once, at the end.
 * On failure it returns 0 and sets ngsLastError; match, scores and sims are untouched. A HIP
 * invalid-value code: NULL match, limit 0, a NaN minSimilarity, an unknown metric or mode, an unknown
 * or un-built hFrom or hTo, ngsCharSize differing between the two, no replica of S on T's device.
 * NGS_ERR_RERANK_LIMIT: limit above 4,096. The arguments are checked before the handles. nS = 0
 * returns 0 without an error. */
#define NGS_LINK_BEST 0u
#define NGS_LINK_ONE_TO_ONE 1u
NGS_API uint32_t linkKeys(uint32_t hFrom, uint32_t hTo, float threshold, uint32_t limit, uint32_t metric,
                          float minSimilarity, uint32_t mode, uint32_t batchKeys, uint32_t* match, float* scores,
                          float* sims);

/* ------------------------------------------------------------------------------------
 * Index sets: several indexes searched as one library, their answers merged on the device (not in
 * the reference).
 *
 * Part. A part p (0 <= p < P <= NGS_SET_MAX_PARTS) is a result block in ngsSearchDevice's layout for
 * the same n queries: dCounts[n], the records of row i at i * stride (a count above the stride is read
 * as the stride), a key base keyBase and a key-length table dKeyLen[nKeys]: the characters of each key
 * as ngsKey / ngsKeyW returns it, without the NUL (ngsKeyLengthsDevice). A record is (p, k, s): part,
 * local key id, fp32 score.
 *
 * Merge order. Records are totally ordered by (1) the order image of the score's fp32 bits
 * descending (as in "Linking two indexes": numeric order for non-NaN floats with -0 < +0, a NaN
 * where its bits put it), (2) dKeyLen[k] ascending, 0xFFFFFFFF for k >= nKeys (nothing is read
 * through such an id), (3) p ascending, (4) k ascending.
 *
 * Output. Row i is the first min(L, sum over p of min(dCounts_p[i], stride_p)) records of the union
 * in that order, L = limit ? limit : 2^31-1, each written as key keyBase_p + k (32-bit arithmetic)
 * with its score bits unchanged. dCounts[i] is that number; cells past it are unspecified; nothing at
 * or beyond i * outStride + outStride is written.
 *
 * Exactness. A key's score depends on its own row only, a result row is ordered by (score
 * descending, key id ascending) and key ids are ranks by (length ascending, first appearance
 * ascending). So for a library cut into contiguous row ranges with no master key in two ranges,
 * indexed one part per range in order, the merge of the parts' answers at (threshold, limit) is bit
 * for bit the answer of one index over all rows, with global key id = keyBase_p + k and keyBase_p
 * the sum of ngsNumKeys of the earlier parts.
 *
 * Precondition. Within a part every row is already in merge order, as ngsSearchDevice writes it. For
 * a row that is not, the order of the output is unspecified; dCounts[i] is still the number above,
 * every access stays in bounds and every written record is one of the inputs.
 *
 * Duplicate keys. Parts are not interned against each other: a master key present in two parts gives
 * two records under two global ids.
 * ------------------------------------------------------------------------------------ */
#define NGS_SET_MAX_PARTS 16u
typedef struct {
    const uint32_t* dCounts; const uint32_t* dKeys; const float* dScores;
    uint32_t stride, keyBase;
    const uint32_t* dKeyLen; uint32_t nKeys;
} ngs_merge_part;

/* dLen[i] = the length of key firstKey + i in characters, from the replica on the current device.
 * Queued on `stream`; nothing waits. 0 ok (nKeys = 0 included); -3 a range past ngsNumKeys or NULL
 * dLen with nKeys > 0 (checked before the handle); -1 bad handle, -2 un-built index, -3 no replica
 * on the current device, -4 HIP error. */
NGS_API int ngsKeyLengthsDevice(uint32_t handle, uint32_t firstKey, uint32_t nKeys, uint32_t* dLen, void* stream);

/* The merge defined above of nParts blocks (`parts` is a host array, read before the call returns)
 * into the caller's block. It takes no handle: the blocks and length tables may come from anywhere,
 * for instance from a gather of other GPUs' blocks. One kernel, no atomics, reproducible bit for bit;
 * queued on `stream`, nothing waits. 0 ok (nQueries = 0 included); -3 NULL parts, nParts 0 or above
 * NGS_SET_MAX_PARTS, nQueries above 2^31-1, NULL outputs with nQueries > 0, a part with NULL
 * dCounts, a part with a non-zero stride and NULL dKeys or dScores, a part with nKeys > 0 and NULL
 * dKeyLen, outStride below min(L, sum of the strides) (the sum in 64 bits); -4 HIP error. */
NGS_API int ngsMergeResultsDevice(const ngs_merge_part* parts, uint32_t nParts, uint32_t nQueries, uint32_t limit,
                                  uint32_t outStride, uint32_t* dCounts, uint32_t* dKeys, float* dScores,
                                  void* stream);

/* A set: 1..NGS_SET_MAX_PARTS built handles searched as one library. Set ids are a namespace of
 * their own (indexN never sees them). All members have one ngsCharSize and one ngsGramSize, every one
 * has a replica on the first member's first device (the set's device), and the sum of their
 * ngsNumKeys is at most 2^32 - 1. Global key id = base_p + k, base_p the sum of ngsNumKeys of the
 * earlier members; ngsSetAdd appends, so global ids are stable under it. The set keeps each member's
 * key-length table on its device (4 bytes a key, built when the member joins). It does not own its
 * members and remembers each by an identity a reused handle id does not share: once a member has been
 * disposed every call on the set answers -1 (the host forms 0 with ngsLastError set) until
 * ngsSetDispose, even if a new index has taken the member's handle id.
 * ngsSetCreate: the set id, or 0 with ngsLastError set (a HIP invalid-value code for a failed
 * condition). ngsSetAdd: 0; -1 unknown set or a disposed member; -3 the set is full or a condition
 * fails; -4 HIP error. ngsSetDispose disposes the set only, never its members. ngsSetParts: the
 * number of members, -1 for an unknown set or a disposed member. ngsSetNumKeys: the total number of
 * keys, 0 likewise. ngsSetLocate: 0 with *handle and *localKey (each may be NULL); -1 likewise; -3
 * keyId >= ngsSetNumKeys. */
NGS_API uint32_t ngsSetCreate(const uint32_t* handles, uint32_t n);
NGS_API int ngsSetAdd(uint32_t set, uint32_t handle);
NGS_API void ngsSetDispose(uint32_t set);
NGS_API int ngsSetParts(uint32_t set);
NGS_API uint32_t ngsSetNumKeys(uint32_t set);
NGS_API int ngsSetLocate(uint32_t set, uint32_t keyId, uint32_t* handle, uint32_t* localKey);

/* ngsSearchDevice over a set: every member searched at (threshold, limit) on the set's device (which
 * must be current) into blocks the call owns, of stride min(L, nKeys_p), then merged into the caller's
 * block; keys are global ids. outStride >= min(L, ngsSetNumKeys). Each member normalises the queries
 * with its own validChar set: a caller who changes one changes them all. Returns when the results
 * are complete. 0; -1 unknown set or a disposed member; -3 as ngsSearchDevice, or the current device
 * is not the set's; -4, -5 as ngsSearchDevice. */
NGS_API int ngsSetSearchDevice(uint32_t set, const uint8_t* dQueryBytes, const uint64_t* dQueryOffsets,
                               uint32_t nQueries, float threshold, uint32_t limit, uint32_t outStride,
                               uint32_t* dCounts, uint32_t* dKeys, float* dScores, void* stream);

/* The host forms, with caller-allocated arrays like selfJoin: counts[nQueries], and the global key
 * ids and scores of query i at i * stride (stride >= min(L, ngsSetNumKeys)). They return the total
 * number of records; on failure 0, the counts zeroed and ngsLastError set. The strings are ngsKey* on
 * what ngsSetLocate answers. scoreBatchSet takes a narrow set, scoreBatchSetW a wide one (0 on a
 * narrow set), scoreBatchSetU8 UTF-8 queries on a wide set. */
NGS_API uint32_t scoreBatchSet(uint32_t set, const char* const* queries, uint32_t nQueries, float threshold,
                               uint32_t limit, uint32_t stride, uint32_t* counts, uint32_t* keyIds, float* scores);
NGS_API uint32_t scoreBatchSetW(uint32_t set, const wchar_t* const* queries, uint32_t nQueries, float threshold,
                                uint32_t limit, uint32_t stride, uint32_t* counts, uint32_t* keyIds, float* scores);
NGS_API uint32_t scoreBatchSetU8(uint32_t set, const char* const* queries, uint32_t nQueries, float threshold,
                                 uint32_t limit, uint32_t stride, uint32_t* counts, uint32_t* keyIds, float* scores);

/* ---- Dead keys: delete from a set without a rebuild ----
 * Definition. A set keeps, per member, a dead mask of one bit per local key id, on its device as it
 * keeps the length tables. Every answer of a set with dead keys is the answer of a set over the same
 * members with the rows of the dead master keys left out, compared by key string, order and fp32 score
 * bits. The global key ids are the unchanged ones of the full set (base_p + k): ids are stable under
 * delete as they are under append. To update a key, remove it and append the new row.
 *
 * Exactness. A key's score depends on its own row only and the whole library's order is (score
 * descending, length ascending, part ascending, local id ascending): removing records from a totally
 * ordered list keeps the order of the rest. The dead records are dropped before a row is cut to the
 * limit, never after it.
 *
 * The members are never changed: a handle searched directly still answers with all its keys, and a
 * handle in two sets has two independent masks. ngsSetNumKeys, ngsSetLocate, ngsKey*,
 * ngsSetKeyQueriesDevice and ngsSetSimilarityDeviceM are unchanged too: a dead key keeps its id and its
 * string, and a record a caller hands in is measured whether its key is dead or not.
 *
 * Searches. A member without dead keys is searched as before, and a set without dead keys launches
 * exactly what it launched before. A member with d dead keys is searched at limit L + E into a block of
 * stride min(L + E, nKeys_p) (the sum in 64 bits; at or above 2^31-1 means all); one ngsDropDeadDevice
 * launch over all such members cuts every row to L, then the merge follows. E starts at min(d, E0),
 * E0 = 128 - L for L <= 112 (the search's fastest tier takes limits up to 128) and max(L, 64) above;
 * the members' short-row counters are read back once (the one extra wait a set with dead keys takes),
 * and a member with short rows whose stride was below both L + d and nKeys_p is searched again with E
 * four times as large, capped at d, where the answer is exact.
 *
 * Self-join and clusters. A dead key is never a hit. The row of a dead query key is empty
 * (ngsSetSelfJoinDevice, selfJoinSet: count 0); dedupKeysSet gives labels[g] = g for a dead g and
 * returns the number of clusters of the live keys.
 *
 * ngsDropDeadDevice: the row rule on a block in ngsSearchDevice's layout, in place. Per row i < n, with
 * c = min(dCounts[i], stride): every record whose key k < nKeys has bit k & 31 of dDead[k >> 5] set is
 * removed (a k >= nKeys is live, nothing is read through it); the remaining records keep their order
 * and move up; the row is cut to L = limit ? limit : 2^31-1; dCounts[i] is the new count. Cells past
 * the new count are unspecified; nothing at or beyond i * stride + stride is written. If dShort is not
 * NULL, *dShort is increased by the number of short rows: rows with c == stride and fewer than L
 * records left, for which the search may have had more hits behind the block. It takes no handle, like
 * ngsDropSelfDevice; one kernel, no atomics on the records, reproducible bit for bit; queued on
 * `stream`, nothing waits. 0 ok (n = 0 included); -3 NULL dCounts, NULL dKeys or dScores with n and
 * stride non-zero, NULL dDead with nKeys > 0, n above 2^31-1; -4 HIP error.
 *
 * ngsSetRemove: the global ids keyIds[n] (a host array) become dead; duplicates and ids already dead
 * are fine. Returns the number of keys newly dead. -3 for an id >= ngsSetNumKeys or NULL keyIds with
 * n > 0, with nothing changed (every id is checked first); -1 unknown set or a disposed member; -4 HIP
 * error. It excludes every other call on the library while it runs, like ngsSetAdd, so a search sees
 * all or none of a call's changes, and the masks on the device are up to date when it returns.
 * ngsSetRestore: the same with the bits cleared; returns the number newly live.
 * ngsSetLiveKeys: the number of live keys (0 for an unknown set). ngsSetDeadKeys: the number of dead
 * keys, their first `cap` global ids written to out ascending (out may be NULL with cap 0): what a
 * caller stores to persist a set's deletions. ngsSetIsLive: 1 or 0; -1; -3 for an id past the set.
 * ngsSetDeadStats: out[0 .. min(n, NGS_SET_DEAD_STATS)) = counters since the set was made: the
 * ngsDropDeadDevice launches of its searches, the member re-searches, the largest over-fetch E used.
 * Returns NGS_SET_DEAD_STATS; -1; -3 n < 0 or NULL out with n > 0. */
#define NGS_SET_DEAD_STATS 3u
NGS_API int ngsDropDeadDevice(uint32_t* dCounts, uint32_t* dKeys, float* dScores, uint32_t n, uint32_t stride,
                              const uint32_t* dDead, uint32_t nKeys, uint32_t limit, uint32_t* dShort, void* stream);
NGS_API int ngsSetRemove(uint32_t set, const uint32_t* keyIds, uint32_t n);
NGS_API int ngsSetRestore(uint32_t set, const uint32_t* keyIds, uint32_t n);
NGS_API uint32_t ngsSetLiveKeys(uint32_t set);
NGS_API uint32_t ngsSetDeadKeys(uint32_t set, uint32_t* out, uint32_t cap);
NGS_API int ngsSetIsLive(uint32_t set, uint32_t keyId);
NGS_API int ngsSetDeadStats(uint32_t set, uint64_t* out, int n);

/* ---- The later stages over a set ----
 * Key ids are the set's global ones everywhere below. Member p owns g iff base_p <= g < base_p +
 * nKeys_p. Every answer is the one a single index over all the members' rows would give (no master
 * key in two members), except that a matched term id is local to the member ngsSetLocate gives for
 * the record's key (ngsTerm on that handle).
 *
 * ngsSetSimilarityDeviceM: ngsSimilarityDeviceM over a set. The similarity of record (i, g) is
 * ngsSimilarityDeviceM's for local key g - base_p on member p, metric, wildcard rule, the 4,096
 * character cap, "a count above the stride reads as the stride" and the fp32 formula included; dTerms
 * (may be NULL) receives the member's local term id, the smallest among equal fp32 values. A g >=
 * ngsSetNumKeys gives -1.0f and 0xFFFFFFFF, nothing read through it. The query is normalised once per
 * query with the validChar set of the set's first member: a caller who changes one member's set
 * changes them all. One kernel launch for the whole block, queued on `stream`; the first call (and the
 * first NGS_SIM_TOKEN_SORT call) builds what a member lacks, as ngsSimilarityDeviceM does, and nothing
 * waits after that. With NGS_SIM_TOKEN_SORT the queries are taken as given (ngsTokenSortDevice on the
 * first member first). -3 NULL arguments as ngsSimilarityDeviceM or an unknown metric (before the set
 * is looked at); -1 unknown set or a disposed member; -3 the current device is not the set's; -4 HIP
 * error. ngsSetRerankDeviceM: that, then ngsRerankDeviceM's filter and order in place; -3 also for
 * stride > 4,096 or a NaN minSimilarity. */
NGS_API int ngsSetSimilarityDeviceM(uint32_t set, const uint8_t* dQueryBytes, const uint64_t* dQueryOffsets,
                                    uint32_t nQueries, uint32_t stride, const uint32_t* dCounts, const uint32_t* dKeys,
                                    uint32_t metric, float* dSim, uint32_t* dTerms, void* stream);
NGS_API int ngsSetRerankDeviceM(uint32_t set, const uint8_t* dQueryBytes, const uint64_t* dQueryOffsets,
                                uint32_t nQueries, uint32_t stride, uint32_t* dCounts, uint32_t* dKeys, float* dScores,
                                float* dSim, uint32_t* dTerms, uint32_t metric, float minSimilarity, void* stream);

/* ngsKeyQueryBytes / ngsKeyQueriesDevice for the global key range [firstKey, firstKey + nKeys), which
 * may span members: the same layout (offsets ascend from 0; on a wide set dBytes is 4-byte aligned),
 * the same return codes with -1 for an unknown set or a disposed member and -3 when the current device
 * is not the set's; nKeys = 0 is valid. ngsSetKeyQueryBytes answers 0 for a bad set or range. */
NGS_API uint64_t ngsSetKeyQueryBytes(uint32_t set, uint32_t firstKey, uint32_t nKeys);
NGS_API int ngsSetKeyQueriesDevice(uint32_t set, uint32_t firstKey, uint32_t nKeys, uint8_t* dBytes, uint64_t capBytes,
                                   uint64_t* dOffsets, void* stream);

/* ngsSelfJoinDevice over a set: the gather above, ngsSetSearchDevice's search at limit + 1, then
 * ngsDropSelfDevice with the global firstKey. outStride >= min((limit ? limit : 2^31-1) + 1,
 * ngsSetNumKeys), else -3. Returns when the results are complete; codes as ngsSelfJoinDevice and
 * ngsSetSearchDevice. */
NGS_API int ngsSetSelfJoinDevice(uint32_t set, uint32_t firstKey, uint32_t nKeys, float threshold, uint32_t limit,
                                 uint32_t outStride, uint32_t* dCounts, uint32_t* dKeys, float* dScores, void* stream);

/* scoreBatchSimM* over a set, with caller-allocated arrays like scoreBatchSet: sims and terms (may be
 * NULL; the members' local term ids) in keyIds' layout. The calls token-sort their own copy of the
 * queries with NGS_SIM_TOKEN_SORT. min(limit ? limit : 2^31-1, ngsSetNumKeys) above 4,096 fails with
 * NGS_ERR_RERANK_LIMIT. selfJoinSet: selfJoin over global ids. dedupKeysSet: dedupKeysM over global ids,
 * labels[ngsSetNumKeys]; batches may cross members; returns the number of clusters. Failure as in the
 * single-index forms: 0, the counts zeroed, ngsLastError set. */
NGS_API uint32_t scoreBatchSetSimM(uint32_t set, const char* const* queries, uint32_t nQueries, float threshold,
                                   uint32_t limit, uint32_t metric, float minSimilarity, uint32_t stride,
                                   uint32_t* counts, uint32_t* keyIds, float* scores, float* sims, uint32_t* terms);
NGS_API uint32_t scoreBatchSetSimMW(uint32_t set, const wchar_t* const* queries, uint32_t nQueries, float threshold,
                                    uint32_t limit, uint32_t metric, float minSimilarity, uint32_t stride,
                                    uint32_t* counts, uint32_t* keyIds, float* scores, float* sims, uint32_t* terms);
NGS_API uint32_t scoreBatchSetSimMU8(uint32_t set, const char* const* queries, uint32_t nQueries, float threshold,
                                     uint32_t limit, uint32_t metric, float minSimilarity, uint32_t stride,
                                     uint32_t* counts, uint32_t* keyIds, float* scores, float* sims, uint32_t* terms);
NGS_API uint32_t selfJoinSet(uint32_t set, uint32_t firstKey, uint32_t nKeys, float threshold, uint32_t limit,
                             uint32_t stride, uint32_t* counts, uint32_t* keyIds, float* scores);
NGS_API uint32_t dedupKeysSet(uint32_t set, float threshold, uint32_t limit, uint32_t metric, float minSimilarity,
                              uint32_t batchKeys, uint32_t* labels);

/* The server of `handle`: 0 none, 1 set up but its kernel not running, 2 its kernel running; -1
 * bad handle (tests). */
NGS_API int ngsServeState(uint32_t handle);

/* Per-call statistics of the last search on `handle` (enable timing first). */
typedef struct {
    uint64_t queries;          /* queries in the call */
    uint64_t fast_queries;     /* handled by the fused LDS kernel */
    uint64_t general_queries;  /* handled by the dense library-wide kernels */
    uint64_t postings;         /* posting ids read by the LDS kernels (k_wave: per gram occurrence) */
    uint64_t lists;            /* posting lists opened */
    uint64_t results;          /* results written by the fused kernel */
    uint64_t survivors;        /* terms whose match ratio passed the threshold (fused kernel) */
    double fast_kernel_ms;     /* fused kernel time from HIP events on the call's stream */
    double prep_kernel_ms;     /* normalisation kernel time */
    double general_ms;         /* general path time (all its kernels) */
    uint64_t handover_queries; /* queries the lean tier-1a kernel handed to the full tier-1b kernel */
    uint64_t tier2_queries;    /* queries routed to the block-per-query tier-2 kernel */
    uint64_t heavy_queries;    /* listed by the prep kernel as heavy (cmin 2: lean kernel on a side stream) */
    uint64_t full_queries;     /* listed by the prep kernel for tier 1b from the start (cmin 1, short search) */
    uint64_t slot_full_queries; /* handed to tier 1b because their survivor slots were full (the
                                   context's slots grow for later calls) */
    uint64_t survivor_slots;   /* survivor slots per query the call ran with */
    uint64_t survivor_slot_bytes; /* bytes of survivor slots and arena the call's context held (rows x
                                     slots x 5 + arena blocks x 1,024 x 5; the slots at most 16 GiB,
                                     and grown slots go back after 16 calls in a row that fill none) */
    uint64_t main_postings;    /* postings and lists of the queries the main tier-1a launch finished */
    uint64_t main_lists;
    uint64_t arena_blocks;     /* survivor arena: blocks (1,024 survivors each) the call's context holds
                                  (queries whose survivors outgrow their slots go on there) */
    uint64_t arena_used;       /* ... blocks the call took (past arena_blocks: it ran out, those
                                  queries went to tier 1b, and later calls get a larger arena) */
} ngs_stats;
NGS_API int ngsSetTiming(uint32_t handle, int enable);
/* The last failure of a call on this thread (0: none); clear != 0 resets it. A HIP error code, or
 * NGS_ERR_INTERNAL (a kernel reported an internal error, the -5 of the device entry points),
 * NGS_ERR_QUERY_BUFFER (a batch outgrew the normalised-query buffer on its rerun) or
 * NGS_ERR_RERANK_LIMIT (scoreBatchSim* with an effective limit above 4,096). A batch split
 * across replicas hands a replica thread's failure to the calling thread. The reference entry
 * points answer 0 on failure, indistinguishable from "no results": a caller that must tell them
 * apart asks here afterwards. */
#define NGS_ERR_INTERNAL 0x10001
#define NGS_ERR_QUERY_BUFFER 0x10002
#define NGS_ERR_RERANK_LIMIT 0x10003 /* scoreBatchSim*: the effective limit is above 4,096 */
NGS_API int ngsLastError(int clear);
NGS_API int ngsLastStats(uint32_t handle, ngs_stats* out);

/* Test support: digests of the index as the kernels read it, for comparing the GPU index build
 * (default) with the host build (environment NGS_HOST_GRAMS=1 / NGS_HOST_INTERN=1 at build time).
 * out[0..7] = postings, lists, skip buckets, FNV-1a of gram_off, post, gram_row, skip, bucket span
 * (gram_off has G + 1 and gram_row G entries: G = 2^21 gram codes for narrow gram size 3, the
 * number of dictionary keys for every other index); out[8..15] = FNV-1a of term_off,
 * term_bytes, tk_off, tk, key_off, key_bytes, wildcard keys, wildcard scores; out[16] = shape flags
 * (1 keys unique, 2 one pair per term, 4 term ids in key-rank order, 8 rank lists: the threshold-0
 * shortcut of indexes with one weight, DevIndex.rank_post); out[17..19] = FNV-1a of the gram
 * dictionary's lookup table as uploaded (ghash_key, ghash_val) and its size in bits (zeros for
 * narrow gram size 3, which has no dictionary). Returns min(n, 20): a caller that passes 17 gets
 * the first 17 words; -1 (bad handle), -4 (HIP error). */
NGS_API int ngsIndexDigest(uint32_t handle, uint64_t* out, int n);
/* The same digests of replica `replica` (0 .. ngsReplicaCount - 1): every replica of an index
 * placed on several devices holds the same arrays. -1 for a bad handle or replica. */
NGS_API int ngsReplicaDigest(uint32_t handle, int replica, uint64_t* out, int n);

/* Index files (an extension; the reference rebuilds on every indexN): ngsSaveIndex writes the
 * interned library of `handle` (terms, term -> (key, weight) pairs, keys, wildcard weights,
 * the validChar set) to `path`: 0, or -1 (bad handle), -2 (unbuilt index), -3 (I/O), -4 (HIP
 * error). ngsLoadIndex builds an index from such a file like indexN builds one from words (the
 * gram CSR is rebuilt; the devices of ngsSetDevices apply): its handle, or 0 if the file cannot
 * be read, is not an index file or is inconsistent. A loaded index answers exactly like the
 * saved one. */
NGS_API int ngsSaveIndex(uint32_t handle, const char* path);
NGS_API uint32_t ngsLoadIndex(const char* path);

/* Library build identification: "ngram_search <version> gfx950 src=<hash>", where <hash> is the
 * first 16 hex digits of the SHA-256 of the sources the library was compiled from. */
NGS_API const char* ngsVersion(void);

/* Diagnostics: the host batch path's phases (scoreBatch / searchBatch / batch score paths of more
 * than 16 queries), nanoseconds summed over the calls since the last reset: [0] query packing,
 * [1] copies in + kernels queued, [2] kernels waited for, [3] device pack + offsets back,
 * [4] records back + marshalling, [5] whole calls, [6] number of calls; [7] the number of
 * one-stream batch calls (all queries heavy, at most 16,384) replayed from a captured graph,
 * any entry point. Writes min(n, 8) values, resets them all if `reset`, returns 8. */
NGS_API int ngsHostPhases(uint64_t* out, int n, int reset);

/* Diagnostics: per-phase time of the LDS kernels (s_memtime shader-clock ticks, summed over
 * waves / blocks) in the instrumented build libngram_search_prof.so; -1 in the regular build. */
NGS_API int ngsPhaseStats(uint64_t* out, int n, int reset);

#ifdef __cplusplus
}
#endif
#endif /* NGRAM_SEARCH_H */
