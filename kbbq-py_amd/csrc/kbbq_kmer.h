// kbbq_kmer.h -- k-mer counting and single-substitution error correction (kbbq correct, kbbq/kmer.py).
//
// Bases A C G T (uppercase only) code as 0 1 2 3; every other byte, and every byte at or beyond the read's length, is a break.
// A k-mer (8 <= k <= 32) is a window of k bases of one read without a break; its key is the smaller of the 2k-bit forward code
// and the reverse-complement code, first base in the high bits.  The all-ones word is never canonical for k <= 32 (its reverse
// complement is 0), so it marks an empty slot.
//
// Table: open addressing over `slots` (a power of two) slots, structure of arrays: keys uint64[slots] (empty = all ones) and
// counts uint32[slots], 12 bytes a slot.  A key's home slot is a 64-bit mix of the key; probing is linear.  Keys are written
// once (empty -> key, by a 64-bit compare-and-swap) and never change, so a plain load that returns a key is final and only an
// empty slot needs the compare-and-swap.  Counts are exact: the table does not depend on thread order.  An insert that finds
// neither its key nor an empty slot within KM_MAX_PROBES probes sets status word ST_KMER and that lane stops inserting; a
// workgroup that starts with the word set inserts nothing.  At the default load factor (<= 0.5) such a run of 512 occupied
// slots does not occur; a table that is too small fails with KBBQ_E_FULL instead of dropping k-mers.  A lookup stops at its
// key, an empty slot or after the same KM_MAX_PROBES probes: every key a successful count inserted lies within that reach.
//
// Work split (every kernel that walks windows): a workgroup takes whole rows, floor(256 / chunks per row) of them (one row when
// a row has more than 256 chunks), and every thread one 16-base chunk at a time.  km_load_chunks turns each chunk into a 32-bit
// code word and a 16-bit break mask in LDS; a thread then reads the words of the next two chunks of its row from LDS (every
// window starting in its chunk ends at most 46 bases later) and handles the 16 windows that start in its chunk: km_walk /
// km_chunk_windows hold that loop, the kernels give it what to do with a window (stage W of km_correct_passes, which skips
// the windows no changed base lies in before it looks at their breaks, keeps a loop of its own).  Each kernel's dynamic LDS
// is a KmLds, from which the host takes the byte count and the kernel its pointers.
//
// Row readers: those kernels are templates over NIB, and only km_load_chunks, km_read_chunk / km_write_chunk / km_chunk_base
// and km_put know it.
// NIB = false: character planes, 16 bytes a chunk.  NIB = true: the 4-bit sequence planes the recalibrate file path keeps
// resident (include/kbbq_hip.h KBBQ_ROWS_NIBBLES: codes A0 T1 G2 C3, 4 = N / separator / padding; 8 bytes a chunk, word w holds
// bases 8w..8w+3 in the low nibbles of its bytes and 8w+4..8w+7 in the high ones).  A nibble >= 4 is a break; the other codes
// map to the table's A0 C1 G2 T3 by swapping 1 and 3, so keys, counts and filter words are those of the character kernels on
// the same bases.  KmerParams.pitch is the plane's row stride in BYTES (half the bases of a row with NIB), cpr the 16-base
// chunks of a row.  A mate-pair row is one row: its separator is a break, no window spans it.
//
// THE RULE (km_decide; stage D of km_correct_passes says the same inline, see there).  A window is valid when it holds no
// break and solid when its k-mer's count is >= min_count; one (solid, valid) bit pair per window lives in LDS (`sv`).  For
// base i of a row:
//   trust         an A/C/G/T base is trusted when a solid window starts in [i - k + 1, i] -- one mask test over the words of the
//                 base's own chunk and the two before it (km_window_bits) -- or when no valid window does.  A trusted base and a
//                 break stay as they are.
//   substitution  an untrusted base takes the letter, of the other three, that makes the most of the valid windows over it
//                 solid (km_vote_subst), when that number is >= 1 and strictly the largest (km_winner); 3 x (covering windows)
//                 lookups.  Otherwise it is unresolved and stays.
//   N rule        (FIXN != KM_FIXN_OFF; KBBQ_KMER_FIX_N) an 'N' (4-bit planes: code 4) inside the read takes the letter that
//                 makes the most of its candidate windows solid -- the windows that cover it, lie inside the read and hold no
//                 other break (km_vote_n: the break masks of chunks ch - 2 .. ch + 2 in LDS) -- by the same pick, of all four.
//                 Which breaks of a chunk are such Ns: km_chunk_ns, from the chunk's bytes.  KM_FIXN_PAIRS: the rows hold two
//                 reads (KBBQ_ROWS_PAIRS), and the base at (length - 1) / 2 is their separator, never an N.  Counting, the
//                 filter and the substitution rule see an N as the break it is.
// Every base is judged against the same state of the row (no cascade inside a pass), so nothing depends on thread order.
// km_decide returns the letter to write, KM_LEAVE or KM_UNRESOLVED; the two kernels differ in where the decision goes:
//   km_correct         judges the row as read and puts the decision into the chunk it holds in registers and then stores
//                      (km_put): the corrected plane, characters or nibbles.  3 LDS words a chunk and a counter a row.
//   ... FLAGS          (kbbq_kmer_flag_dev) KmerParams.out is a flag plane of the input's geometry, one byte a base: 1 where the
//                      correction would write another letter, 0 everywhere else -- breaks, trusted bases, ties, padding.  The
//                      chunk starts as zeros instead of the bytes read and is stored whatever it holds: every byte is written.
//   ... UNRES          (KBBQ_KMER_FLAG_UNRESOLVED) KM_UNRESOLVED becomes 2 in the flag plane (km_flag), the skip bit of the aligned
//                      tally.  A byte is 0, 1 or 2, never 3.  The row's counter in LDS holds the 1s in its low and the 2s in its
//                      high 16 bits (a row has at most 65535 bases, and a base is one or the other); KmerParams.unresolved
//                      receives the high half.
//   ... TALLY          (kbbq_kmer_correct_rows_skip_dev) the corrected form's own third outcome: the corrected plane is what it is
//                      without, and KM_UNRESOLVED goes to a second QUALITY plane, the tally plane (KmerTally): the chunk's 16
//                      quality bytes as read with 0 at every unresolved base (km_tally_chunk).  K1 sends a base of quality byte
//                      < 33 + minscore to its trash row and looks at the base's own byte alone, so the tally leaves out exactly
//                      those bases and K1 needs no flag plane.  Quality planes are characters, [nrows, 16 cpr], also beside a
//                      4-bit sequence plane.  Every byte of every row is written; the counter splits as with UNRES.
//   km_correct_passes  keeps the row in LDS and applies the rule to its own output up to `passes` times: the decisions of a
//                      pass go to a second copy of the row's code words and break masks.  See the comment at the kernel.
//
// Ranks (kbbq/kmer.py count_kmers_ranks): the owner of a canonical key among W ranks is km_owner(key, W), the high 32 bits of
// the same mix taken of the key XOR a constant, scaled to 0..W-1.  It shares no bits with the home slot (km_hash(key) & mask),
// so the keys one rank owns spread over all home slots of its table.  km_select_sizes / km_select_scatter sort the occupied
// slots with count >= min_count into buckets by owner (one bucket: compaction), km_merge adds (key, count) pairs to a table
// through km_insert, as km_count adds 1.
//
// Prefilter (kbbq correct --prefilter): a filter is two arrays of `words` (a power of two) 64-bit words, `seen` and `twice`.
// A canonical key has one word index and one mask of up to 4 bits, the same in both arrays (km_filter_index).  km_prefilter
// ORs the mask into seen[word]; a key whose mask was whole there before its OR (the key, or a false positive, came before) ORs it
// into twice[word], and an OR into `twice` that set a new bit adds one to `admitted`.  Both tests of a window read the value
// ONE atomic returned, so of the occurrences of a key at most one finds its mask incomplete: every key that occurs twice or
// more is in `twice`, whatever the thread order.  Bits are only ever set, so a relaxed load that shows the whole mask is
// final and the atomic is skipped.  km_count_filtered is km_count for the windows whose mask is whole in `twice`: the table
// then holds every key of count >= 2 with its exact count and some keys of count 1 (false positives), nothing else.
//
// Quality gate (kbbq correct --kmer-min-qual Q): km_gate, at the end of this file, writes a copy of the sequence plane with a
// break wherever the quality byte is below the threshold and counts the windows that are left; every counting kernel above
// reads that copy as it reads any plane.
#pragma once
#include "kbbq_helpers.h"

constexpr int KM_THREADS = 256;
constexpr u64 KM_EMPTY = ~0ull;
constexpr int KM_HIST = 257;          // h[c], c = 1..255; h[256]: count >= 256; h[0] stays 0
constexpr int KM_FIXN_OFF = 0, KM_FIXN_READS = 1, KM_FIXN_PAIRS = 2;   // km_correct's N rule: off, one read a row, two reads a row

struct KmerParams {
    const uint8_t* seq; const u32* meta; int64_t nrows; int pitch; int cpr; int rows_per_wg; int k;   // pitch: row stride, bytes
    u64* keys; u32* counts; u64 mask;
    u32 min_count;                    // correct: a k-mer is solid when its count is >= min_count
    uint8_t* out; u32* changed;       // correct: the corrected plane (flag form: the flag plane); per-row count of changed bases (may be NULL)
    u64* status;
    u32* unresolved;                  // UNRES / TALLY: per-row count of unresolved bases (may be NULL)
};

// the correction kernels' last parameter, read by the TALLY forms alone: the quality plane as read and the tally plane, both
// [nrows, 16 cpr] characters and 16-byte aligned
struct KmerTally { const uint8_t* qual; uint8_t* out; };

__host__ __device__ __forceinline__ u64 km_hash(u64 x)
{
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

// reverse complement of a 2k-bit forward code
__device__ __forceinline__ u64 km_revcomp(u64 f, int k)
{
    u64 y = __builtin_bitreverse64(~f);                                   // complement, groups reversed (bits swapped in each)
    y = ((y >> 1) & 0x5555555555555555ull) | ((y & 0x5555555555555555ull) << 1);
    return y >> (64 - 2 * k);
}

__device__ __forceinline__ u64 km_canonical(u64 f, int k)
{
    const u64 r = km_revcomp(f, k);
    return f < r ? f : r;
}

__device__ __forceinline__ u64 km_load_key(const u64* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// count of `key`, 0 when absent
__device__ __forceinline__ u32 km_lookup(const KmerParams& p, u64 key)
{
    u64 s = km_hash(key) & p.mask;
    for (int i = 0; i < KM_MAX_PROBES; ++i) {
        const u64 cur = km_load_key(p.keys + s);
        if (cur == key) return p.counts[s];
        if (cur == KM_EMPTY) return 0;
        s = (s + 1) & p.mask;
    }
    return 0;
}

// counts[key] += add; false when neither the key nor an empty slot lies within KM_MAX_PROBES probes
__device__ __forceinline__ bool km_insert(u64* keys, u32* counts, u64 mask, u64 key, u32 add)
{
    u64 s = km_hash(key) & mask;
    bool done = false;
    for (int i = 0; i < KM_MAX_PROBES && !done; ++i) {
        u64 cur = km_load_key(keys + s);
        if (cur == KM_EMPTY) {
            cur = atomicCAS(keys + s, KM_EMPTY, key);
            if (cur == KM_EMPTY) cur = key;                               // this lane claimed the slot
        }
        if (cur == key) { atomicAdd(counts + s, add); done = true; }
        s = (s + 1) & mask;
    }
    return done;
}

// ---- dynamic LDS of the kernels that walk windows: `chunk` arrays of one word per chunk of the workgroup's rows, then `row`
// arrays of one word per row, then `wg` single words.  The host takes the byte count and the kernels their pointers from here.
struct KmLds { int chunk, row, wg; };
constexpr KmLds KM_LDS_COUNT = {2, 0, 0};       // km_count, km_count_filtered: code, brk
constexpr KmLds KM_LDS_PREFILTER = {2, 0, 1};   // km_prefilter: code, brk; the workgroup's `admitted`
constexpr KmLds KM_LDS_CORRECT = {3, 1, 0};     // km_correct: code, brk, sv; nchg
constexpr KmLds KM_LDS_PASSES = {8, 2, 1};      // km_correct_passes: code0, brk0, (code, brk) twice, sv, mark; nchg, last; wglast

__host__ __device__ __forceinline__ size_t km_lds_bytes(KmLds l, int rows_per_wg, int cpr)
{
    return ((size_t)l.chunk * rows_per_wg * cpr + (size_t)l.row * rows_per_wg + l.wg) * 4;
}
__device__ __forceinline__ u32* km_lds_chunk(u32* lds, const KmerParams& p, int i) { return lds + i * p.rows_per_wg * p.cpr; }
__device__ __forceinline__ u32* km_lds_row(u32* lds, KmLds l, const KmerParams& p, int i)
{
    return lds + l.chunk * p.rows_per_wg * p.cpr + i * p.rows_per_wg;
}
__device__ __forceinline__ u32* km_lds_wg(u32* lds, KmLds l, const KmerParams& p) { return km_lds_row(lds, l, p, l.row); }

// the table's code (A0 C1 G2 T3) of a plane nibble 0..3 (A0 T1 G2 C3) and back: 1 and 3 change places
__device__ __forceinline__ u32 km_nib_swap(u32 n) { return n ^ ((n & 1u) << 1); }

// bit offset of base t (0..7) of a word of a 4-bit plane
__device__ __forceinline__ int km_nib_shift(int t) { return 8 * (t & 3) + 4 * ((t >> 2) & 1); }

// byte offset in the plane of chunk ch of a row: a chunk is 8 bytes of nibbles or 16 of characters
template <bool NIB>
__device__ __forceinline__ size_t km_chunk_at(const KmerParams& p, int64_t row, int ch)
{
    return (size_t)row * p.pitch + (size_t)ch * (NIB ? 8 : 16);
}

// the chunk at `at` as 4 words of characters or 2 of nibbles; FLAGS: a chunk of the flag plane instead, all 0, nothing to read
template <bool NIB, bool FLAGS = false>
__device__ __forceinline__ void km_read_chunk(const uint8_t* at, u32 (&w)[4])
{
    w[0] = w[1] = w[2] = w[3] = 0;
    if constexpr (FLAGS) {
    } else if constexpr (NIB) {
        const uint2 v = *reinterpret_cast<const uint2*>(at);
        w[0] = v.x; w[1] = v.y;
    } else {
        const uint4 v = *reinterpret_cast<const uint4*>(at);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    }
}

template <bool NIB>
__device__ __forceinline__ void km_write_chunk(uint8_t* at, const u32 (&w)[4])
{
    if constexpr (NIB) *reinterpret_cast<uint2*>(at) = make_uint2(w[0], w[1]);
    else *reinterpret_cast<uint4*>(at) = make_uint4(w[0], w[1], w[2], w[3]);
}

// base t of a chunk as the plane holds it: a character or a nibble
template <bool NIB>
__device__ __forceinline__ u32 km_chunk_base(const u32 (&w)[4], int t)
{
    return NIB ? (w[t >> 3] >> km_nib_shift(t & 7)) & 0xFu : (w[t >> 2] >> (8 * (t & 3))) & 0xFFu;
}

// Pass 1: the code word (base t of the chunk in bits 31 - 2t .. 30 - 2t) and break mask (bit t) of every chunk of the
// workgroup's rows.  Returns the number of rows this workgroup holds.
template <bool NIB>
__device__ __forceinline__ int km_load_chunks(const KmerParams& p, int64_t row0, u32* code, u32* brk)
{
    const int nr = (int)(p.nrows - row0 < p.rows_per_wg ? p.nrows - row0 : p.rows_per_wg);
    for (int e = threadIdx.x; e < nr * p.cpr; e += KM_THREADS) {
        const int r = e / p.cpr, ch = e - r * p.cpr;
        const int64_t row = row0 + r;
        const int L = (int)(p.meta[row] & 0xFFFFu);
        u32 c = 0, b = 0;
        if constexpr (NIB) {
            const uint2 v = *reinterpret_cast<const uint2*>(p.seq + (size_t)row * p.pitch + (size_t)ch * 8);
            const u32 w[2] = {v.x, v.y};
            #pragma unroll
            for (int t = 0; t < 16; ++t) {
                const u32 x = (w[t >> 3] >> km_nib_shift(t & 7)) & 0xFu;
                const bool base = x < 4u && ch * 16 + t < L;
                c |= (base ? km_nib_swap(x) : 0u) << (30 - 2 * t);
                b |= (base ? 0u : 1u) << t;
            }
        } else {
            const uint4 v = *reinterpret_cast<const uint4*>(p.seq + (size_t)row * p.pitch + (size_t)ch * 16);
            const u32 w[4] = {v.x, v.y, v.z, v.w};
            #pragma unroll
            for (int t = 0; t < 16; ++t) {
                const u32 x = (w[t >> 2] >> (8 * (t & 3))) & 0xFFu;
                const u32 cv = x == 'A' ? 0u : x == 'C' ? 1u : x == 'G' ? 2u : 3u;
                const bool base = (x == 'A' || x == 'C' || x == 'G' || x == 'T') && ch * 16 + t < L;
                c |= (base ? cv : 0u) << (30 - 2 * t);
                b |= (base ? 0u : 1u) << t;
            }
        }
        code[e] = c; brk[e] = b;
    }
    return nr;
}

// the code words of chunks ch .. ch + n - 1 of a row as one big-endian 128-bit word (chunks past the row: code 0, all breaks)
__device__ __forceinline__ unsigned __int128 km_words(const KmerParams& p, const u32* code, const u32* brk, int e_row, int ch,
                                                      int n, u64* breaks)
{
    unsigned __int128 x = 0; u64 b = 0;
    for (int i = 0; i < n; ++i) {
        const int c = ch + i;
        const bool in = c >= 0 && c < p.cpr;
        x |= (unsigned __int128)(in ? code[e_row + c] : 0u) << (96 - 32 * i);
        b |= (u64)(in ? brk[e_row + c] : 0xFFFFu) << (16 * i);
    }
    *breaks = b;
    return x;
}

// forward code of the window that starts `o` bases into a 128-bit word
__device__ __forceinline__ u64 km_window(unsigned __int128 x, int o, int k)
{
    return (u64)((x << (2 * o)) >> (128 - 2 * k));
}

// The window walk.  km_chunk_windows: f(o, forward code) for every window without a break that starts o bases into chunk ch of
// the row at e_row; f returns whether to go on, and so does the walk.  km_walk: f(r, e, o, forward code) for every such window
// of the workgroup's nr rows, a thread taking chunks e = threadIdx.x, + KM_THREADS, ... (r: the row in the workgroup).
template <class F>
__device__ __forceinline__ bool km_chunk_windows(const KmerParams& p, const u32* code, const u32* brk, int e_row, int ch, F&& f)
{
    const u64 kmask = (1ull << p.k) - 1;
    u64 b;
    const unsigned __int128 x = km_words(p, code, brk, e_row, ch, 3, &b);
    for (int o = 0; o < 16; ++o) {
        if ((b >> o) & kmask) continue;
        if (!f(o, km_window(x, o, p.k))) return false;
    }
    return true;
}

template <class F>
__device__ __forceinline__ void km_walk(const KmerParams& p, const u32* code, const u32* brk, int nr, F&& f)
{
    for (int e = threadIdx.x; e < nr * p.cpr; e += KM_THREADS) {
        const int r = e / p.cpr, ch = e - r * p.cpr;
        if (!km_chunk_windows(p, code, brk, r * p.cpr, ch, [&](int o, u64 w) { return f(r, e, o, w); })) return;
    }
}

__device__ __forceinline__ bool km_table_full(const KmerParams& p)
{
    return __hip_atomic_load(p.status + ST_KMER, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != ~0ull;
}

template <bool NIB>
__global__ __launch_bounds__(KM_THREADS) void km_count(KmerParams p)
{
    extern __shared__ u32 km_lds[];
    u32* code = km_lds_chunk(km_lds, p, 0); u32* brk = km_lds_chunk(km_lds, p, 1);
    const int64_t row0 = (int64_t)blockIdx.x * p.rows_per_wg;
    const int nr = km_load_chunks<NIB>(p, row0, code, brk);
    __syncthreads();
    if (km_table_full(p)) return;
    km_walk(p, code, brk, nr, [&](int r, int, int, u64 f) {
        if (km_insert(p.keys, p.counts, p.mask, km_canonical(f, p.k), 1u)) return true;
        atomicMin(p.status + ST_KMER, (u64)(row0 + r));
        return false;
    });
}

// ---- prefilter: keys seen once stay out of the table ---------------------------------------------------------------------------
constexpr u64 KM_FILTER_SALT = 0xD6E8FEB86659FD93ull;

struct KmerFilterParams {
    u64* seen; u64* twice; u64 wmask;  // words - 1
    u64* admitted;                     // OR-operations into `twice` that set a new bit
};

// word index and mask of a canonical key: 4 six-bit fields of the low 24 bits of the mix pick the bits, the bits above the word
__host__ __device__ __forceinline__ u64 km_filter_index(u64 key, u64 wmask, u64* mask)
{
    const u64 h = km_hash(key ^ KM_FILTER_SALT);
    *mask = 1ull << (h & 63) | 1ull << ((h >> 6) & 63) | 1ull << ((h >> 12) & 63) | 1ull << ((h >> 18) & 63);
    return (h >> 24) & wmask;
}

// OR `mask` into *p unless a load shows it whole already; the value before (a load that shows the mask whole is that value)
__device__ __forceinline__ u64 km_filter_or(u64* p, u64 mask)
{
    const u64 cur = km_load_key(p);
    return (cur & mask) == mask ? cur : atomicOr(p, mask);
}

template <bool NIB>
__global__ __launch_bounds__(KM_THREADS) void km_prefilter(KmerParams p, KmerFilterParams f)
{
    extern __shared__ u32 km_lds[];
    u32* code = km_lds_chunk(km_lds, p, 0); u32* brk = km_lds_chunk(km_lds, p, 1);
    u32* adm = km_lds_wg(km_lds, KM_LDS_PREFILTER, p);
    const int64_t row0 = (int64_t)blockIdx.x * p.rows_per_wg;
    if (threadIdx.x == 0) *adm = 0;
    const int nr = km_load_chunks<NIB>(p, row0, code, brk);
    __syncthreads();
    u32 mine = 0;
    km_walk(p, code, brk, nr, [&](int, int, int, u64 fw) {
        u64 m;
        const u64 w = km_filter_index(km_canonical(fw, p.k), f.wmask, &m);
        if ((km_filter_or(f.seen + w, m) & m) != m) return true;          // first of its mask
        if ((km_filter_or(f.twice + w, m) & m) != m) ++mine;
        return true;
    });
    if (mine) atomicAdd(adm, mine);
    __syncthreads();
    if (threadIdx.x == 0 && *adm) atomicAdd(f.admitted, (u64)*adm);
}

// km_count of the windows whose mask is whole in `twice`
template <bool NIB>
__global__ __launch_bounds__(KM_THREADS) void km_count_filtered(KmerParams p, KmerFilterParams f)
{
    extern __shared__ u32 km_lds[];
    u32* code = km_lds_chunk(km_lds, p, 0); u32* brk = km_lds_chunk(km_lds, p, 1);
    const int64_t row0 = (int64_t)blockIdx.x * p.rows_per_wg;
    const int nr = km_load_chunks<NIB>(p, row0, code, brk);
    __syncthreads();
    if (km_table_full(p)) return;
    km_walk(p, code, brk, nr, [&](int r, int, int, u64 fw) {
        const u64 key = km_canonical(fw, p.k);
        u64 m;
        const u64 w = km_filter_index(key, f.wmask, &m);
        if ((f.twice[w] & m) != m) return true;                           // seen once
        if (km_insert(p.keys, p.counts, p.mask, key, 1u)) return true;
        atomicMin(p.status + ST_KMER, (u64)(row0 + r));
        return false;
    });
}

// h[min(count, 256)] += 1 for every occupied slot
__global__ __launch_bounds__(KM_THREADS) void km_histogram(const u64* keys, const u32* counts, u64 slots, u64* hist)
{
    __shared__ u32 h[KM_HIST];
    for (int i = threadIdx.x; i < KM_HIST; i += KM_THREADS) h[i] = 0;
    __syncthreads();
    const u64 stride = (u64)gridDim.x * KM_THREADS;
    for (u64 s = (u64)blockIdx.x * KM_THREADS + threadIdx.x; s < slots; s += stride)
        if (keys[s] != KM_EMPTY) atomicAdd(&h[min(counts[s], 256u)], 1u);
    __syncthreads();
    for (int i = threadIdx.x; i < KM_HIST; i += KM_THREADS)
        if (h[i]) atomicAdd(hist + i, (u64)h[i]);
}

__device__ __forceinline__ bool km_solid(const KmerParams& p, u64 f)
{
    return km_lookup(p, km_canonical(f, p.k)) >= p.min_count;
}

// the 16 break masks of chunks ch .. ch + n - 1 of a row (n <= 8), chunk ch in the low bits; chunks past the row: all breaks
__device__ __forceinline__ unsigned __int128 km_breaks(const KmerParams& p, const u32* brk, int e_row, int ch, int n)
{
    unsigned __int128 b = 0;
    for (int i = 0; i < n; ++i) {
        const int c = ch + i;
        b |= (unsigned __int128)(c >= 0 && c < p.cpr ? brk[e_row + c] : 0xFFFFu) << (16 * i);
    }
    return b;
}

// ---- the correction rule, one base at a time --------------------------------------------------------------------------------
// What a thread holds while it judges the 16 bases of chunk ch of the row whose words start at e_row of code / brk.
// Positions count from the first base of chunk ch - 2: base t of the chunk is position 32 + t, window j starts at position j.
struct KmChunk {
    const u32* code; const u32* brk; int e_row, ch;
    u32 brk_own;                                     // brk[e_row + ch]
    u32 ns;                                          // N rule: bit t, base t is an N the rule may fix (km_chunk_ns)
    u64 V, S;                                        // bit j: window j is valid, is solid (km_window_bits)
    bool have_words; unsigned __int128 xa, xb;       // the code words of chunks ch - 2 .. ch + 1 and ch .. ch + 3 (km_context)
};

// bit t: base t of the chunk `w` is an N ('N', code 4 of a 4-bit plane) inside the read and not the separator of two reads
template <bool NIB, int FIXN>
__device__ __forceinline__ u32 km_chunk_ns(const KmerParams& p, const u32 (&w)[4], u32 brk_own, int64_t row, int ch)
{
    u32 ns = 0;
    #pragma unroll
    for (int t = 0; t < 16; ++t) ns |= (km_chunk_base<NIB>(w, t) == (NIB ? 4u : (u32)'N') ? 1u : 0u) << t;
    ns &= brk_own;
    if (ns) {
        const int L = (int)(p.meta[row] & 0xFFFFu), first = ch * 16;
        ns &= L - first >= 16 ? 0xFFFFu : L > first ? (1u << (L - first)) - 1u : 0u;
        const int sep = FIXN == KM_FIXN_PAIRS ? ((L - 1) >> 1) - first : -1;
        if (sep >= 0 && sep < 16) ns &= ~(1u << sep);
    }
    return ns;
}

// the (solid << 16 | valid) words `sv` of chunks ch - 2 .. ch as two 48-bit masks
__device__ __forceinline__ void km_window_bits(const u32* sv, int e_row, int ch, u64* V, u64* S)
{
    *V = 0; *S = 0;
    for (int i = 0; i < 3; ++i) {
        const int c = ch - 2 + i;
        const u32 w = c >= 0 ? sv[e_row + c] : 0u;
        *V |= (u64)(w & 0xFFFFu) << (16 * i);
        *S |= (u64)(w >> 16) << (16 * i);
    }
}

// xa, xb on first use: most chunks need neither
__device__ __forceinline__ void km_context(const KmerParams& p, KmChunk& c)
{
    if (c.have_words) return;
    u64 unused;
    c.xa = km_words(p, c.code, c.brk, c.e_row, c.ch - 2, 4, &unused);
    c.xb = km_words(p, c.code, c.brk, c.e_row, c.ch, 4, &unused);
    c.have_words = true;
}

// forward code of window j with `x` XOR-ed into the base at position pp
__device__ __forceinline__ u64 km_window_with(const KmerParams& p, const KmChunk& c, int j, int pp, u32 x)
{
    return (j < 32 ? km_window(c.xa, j, p.k) : km_window(c.xb, j - 32, p.k)) ^ ((u64)x << (2 * (p.k - 1 - (pp - j))));
}

// N rule: s[x] = the candidate windows of the N at base t -- it is their only break -- that letter x makes solid
__device__ __forceinline__ void km_vote_n(const KmerParams& p, const KmChunk& c, int t, int (&s)[4])
{
    const u64 kmask = (1ull << p.k) - 1;
    const unsigned __int128 B = km_breaks(p, c.brk, c.e_row, c.ch - 2, 5);   // bit i: the base at position i
    const int pp = 32 + t;
    for (int j = pp - p.k + 1; j <= pp; ++j) {
        if (((u64)(B >> j) & kmask) != 1ull << (pp - j)) continue;
        #pragma unroll
        for (u32 x = 0; x < 4; ++x) s[x] += km_solid(p, km_window_with(p, c, j, pp, x)) ? 1 : 0;   // a break's code is 0
    }
}

// substitution rule: s[alt] = the valid windows over base t (`windows`: V & cover) that letter alt in place of orig makes solid
__device__ __forceinline__ void km_vote_subst(const KmerParams& p, const KmChunk& c, int t, u32 orig, u64 windows, int (&s)[4])
{
    for (u32 alt = 0; alt < 4; ++alt) {
        if (alt == orig) continue;
        for (u64 m = windows; m; m &= m - 1)
            s[alt] += km_solid(p, km_window_with(p, c, __builtin_ctzll(m), 32 + t, orig ^ alt)) ? 1 : 0;
    }
}

// the letter with the strictly largest score >= 1 (`skip` left out), -1 when there is none
__device__ __forceinline__ int km_winner(const int (&s)[4], int skip)
{
    int best = -1, bs = 0; bool tie = false;
    #pragma unroll
    for (int x = 0; x < 4; ++x) {
        if (x == skip) continue;
        if (s[x] > bs) { bs = s[x]; best = x; tie = false; }
        else if (s[x] == bs && bs > 0) tie = true;
    }
    return tie ? -1 : best;
}

// The rule for base t: the table's code 0..3 to write (a fixed N also stops being a break), or
constexpr int KM_LEAVE = -1;                         // a break, a trusted base, an N no letter wins
constexpr int KM_UNRESOLVED = -2;                    // an untrusted base no substitution wins

template <int FIXN>
__device__ __forceinline__ int km_decide(const KmerParams& p, KmChunk& c, int t)
{
    if constexpr (FIXN != KM_FIXN_OFF) {
        if ((c.ns >> t) & 1u) {
            int s[4] = {0, 0, 0, 0};
            km_context(p, c);
            km_vote_n(p, c, t, s);
            const int best = km_winner(s, -1);
            return best < 0 ? KM_LEAVE : best;
        }
    }
    if ((c.brk_own >> t) & 1u) return KM_LEAVE;                           // a break: never changed
    const u64 cover = ((1ull << p.k) - 1) << (32 + t - p.k + 1);
    if ((c.S & cover) || !(c.V & cover)) return KM_LEAVE;                 // trusted
    km_context(p, c);
    const u32 orig = (c.code[c.e_row + c.ch] >> (30 - 2 * t)) & 3u;
    int s[4] = {0, 0, 0, 0};
    km_vote_subst(p, c, t, orig, c.V & cover, s);
    const int best = km_winner(s, (int)orig);
    return best < 0 ? KM_UNRESOLVED : best;
}

// the byte of base t of a chunk of the flag plane (all 0 before) becomes v: 1 error, 2 unresolved
__device__ __forceinline__ void km_flag(u32 (&w)[4], int t, u32 v) { w[t >> 2] |= v << (8 * (t & 3)); }

// The store stage: base t of the chunk `w` (4 words of characters, 2 of nibbles) takes the table's code `best`.
// FLAGS: `w` is the chunk of the flag plane instead, one byte a base, and the base's byte becomes 1.
template <bool NIB, bool FLAGS>
__device__ __forceinline__ void km_put(u32 (&w)[4], int t, u32 best)
{
    if constexpr (FLAGS) {
        km_flag(w, t, 1u);
    } else if constexpr (NIB) {
        const int sh = km_nib_shift(t & 7);
        w[t >> 3] = (w[t >> 3] & ~(0xFu << sh)) | (km_nib_swap(best) << sh);
    } else {
        const u32 letter = best == 0 ? 'A' : best == 1 ? 'C' : best == 2 ? 'G' : 'T';
        const int sh = 8 * (t & 3);
        w[t >> 2] = (w[t >> 2] & ~(0xFFu << sh)) | (letter << sh);
    }
}

// TALLY: the 16 quality bytes of a chunk go to the tally plane, 0 where `un` (bit t: base t is unresolved) says so.  seq_at: the
// chunk's km_chunk_at in the sequence plane; a quality plane has 16 bytes a chunk, so the chunk lies at twice that beside nibbles
template <bool NIB>
__device__ __forceinline__ void km_tally_chunk(const KmerTally& q, size_t seq_at, u32 un)
{
    const size_t at = NIB ? 2 * seq_at : seq_at;
    const uint4 v = *reinterpret_cast<const uint4*>(q.qual + at);
    u32 w[4] = {v.x, v.y, v.z, v.w};
    #pragma unroll
    for (int i = 0; i < 4; ++i) {
        const u32 m = (un >> (4 * i)) & 0xFu;                             // bit j -> byte j: 0xFF where the base is unresolved
        w[i] &= ~((((m & 1u) | (m & 2u) << 7 | (m & 4u) << 14 | (m & 8u) << 21)) * 0xFFu);
    }
    *reinterpret_cast<uint4*>(q.out + at) = make_uint4(w[0], w[1], w[2], w[3]);
}

// nchg[row] to KmerParams.changed / .unresolved.  SPLIT: changed bases in the low half, unresolved ones in the high half;
// else the whole word counts changed bases (up to 65535: the high half is 0) and .unresolved is not looked at
template <bool SPLIT>
__device__ __forceinline__ void km_flush_counts(const KmerParams& p, int64_t row0, int nr, const u32* nchg)
{
    if (!p.changed && !(SPLIT && p.unresolved)) return;
    __syncthreads();
    for (int i = threadIdx.x; i < nr; i += KM_THREADS) {
        if (p.changed) p.changed[row0 + i] = SPLIT ? nchg[i] & 0xFFFFu : nchg[i];
        if (SPLIT && p.unresolved) p.unresolved[row0 + i] = nchg[i] >> 16;
    }
}

template <bool NIB, int FIXN = KM_FIXN_OFF, bool FLAGS = false, bool UNRES = false, bool TALLY = false>
__global__ __launch_bounds__(KM_THREADS) void km_correct(KmerParams p, KmerTally q)
{
    static_assert(!FLAGS || (!NIB && FIXN == KM_FIXN_OFF), "the flag form: character rows, no N rule");
    static_assert(!UNRES || FLAGS, "unresolved bases are a value of the flag plane: the flag form only");
    static_assert(!TALLY || !FLAGS, "the tally plane goes with the corrected plane: the corrected form only");
    extern __shared__ u32 km_lds[];
    u32* code = km_lds_chunk(km_lds, p, 0); u32* brk = km_lds_chunk(km_lds, p, 1); u32* sv = km_lds_chunk(km_lds, p, 2);
    u32* nchg = km_lds_row(km_lds, KM_LDS_CORRECT, p, 0);
    const int64_t row0 = (int64_t)blockIdx.x * p.rows_per_wg;
    for (int i = threadIdx.x; i < p.rows_per_wg; i += KM_THREADS) nchg[i] = 0;
    const int nr = km_load_chunks<NIB>(p, row0, code, brk);
    __syncthreads();
    // pass 2: (solid << 16 | valid) of the 16 windows starting in every chunk
    for (int e = threadIdx.x; e < nr * p.cpr; e += KM_THREADS) {
        const int r = e / p.cpr, ch = e - r * p.cpr;
        u32 valid = 0, solid = 0;
        km_chunk_windows(p, code, brk, r * p.cpr, ch, [&](int o, u64 f) {
            valid |= 1u << o;
            if (km_solid(p, f)) solid |= 1u << o;
            return true;
        });
        sv[e] = solid << 16 | valid;
    }
    __syncthreads();
    // pass 3: the rule for every base of the chunk as read; the decisions go into the chunk in registers
    for (int e = threadIdx.x; e < nr * p.cpr; e += KM_THREADS) {
        const int r = e / p.cpr, ch = e - r * p.cpr;
        const size_t at = km_chunk_at<NIB>(p, row0 + r, ch);
        u32 w[4];
        km_read_chunk<NIB, FLAGS>(p.seq + at, w);
        KmChunk c = {code, brk, r * p.cpr, ch, brk[e], 0, 0, 0, false, 0, 0};
        km_window_bits(sv, c.e_row, ch, &c.V, &c.S);
        if constexpr (FIXN != KM_FIXN_OFF) c.ns = km_chunk_ns<NIB, FIXN>(p, w, c.brk_own, row0 + r, ch);
        int changed = 0, unres = 0;
        u32 un = 0;                                                       // TALLY: bit t, base t is unresolved
        for (int t = 0; t < 16; ++t) {
            const int d = km_decide<FIXN>(p, c, t);
            if (d >= 0) { km_put<NIB, FLAGS>(w, t, (u32)d); ++changed; }
            else if (UNRES && d == KM_UNRESOLVED) { km_flag(w, t, 2u); ++unres; }
            else if (TALLY && d == KM_UNRESOLVED) un |= 1u << t;
        }
        km_write_chunk<NIB>(p.out + at, w);
        if constexpr (TALLY) { km_tally_chunk<NIB>(q, at, un); unres = __popc(un); }
        if (changed | unres) atomicAdd(&nchg[r], (u32)changed | (u32)unres << 16);
    }
    km_flush_counts<UNRES || TALLY>(p, row0, nr, nchg);
}

// ---- several passes of the rule over rows held in LDS (kbbq correct --passes; include/kbbq_hip.h kbbq_kmer_*_passes*) ----------
// r_0 is the row as read and r_p = C(r_(p-1)), C being the rule above (with FIXN the N rule too) against the same table at
// the same min_count: nothing is recounted.  km_correct's work split and pass 1; then the row lives in LDS until it is stored:
//   code0 / brk0      the chunk as read (brk0's high half: the Ns of the read the N rule may fix -- inside the read, no separator)
//   codeA/brkA, codeB/brkB   r_(p-1) and r_p: a pass reads one copy and writes the other, the copies swap after a barrier, so no
//                     base sees a decision of its own pass
//   sv                (solid << 16 | valid) of the 16 windows starting in the chunk, as km_correct's
//   mark              low half: the bases of the chunk the row's last pass changed; high half: those it left unresolved
//   nchg[row]         km_correct's counters;  last[row]: the last pass that changed the row;  wglast: ... any row of the workgroup
// From pass 2 on a window is looked up again only when a base the pass before changed lies in it (a fixed N changes validity
// too, and is such a base); every other window keeps its bits.  A row whose pass p - 1 changed nothing is skipped from pass p on
// (both copies hold it then), and the workgroup leaves the loop after a pass in which none of its rows changed: every thread
// reads that from wglast after the barrier, so the trip count is uniform and every __syncthreads() is reached by all threads.
// The store stage writes km_put's form wherever the final copy differs from code0 / brk0, and with UNRES 2 where it does not
// and the row's last pass left the base unresolved (TALLY: those bases are the zeros of the tally plane instead, km_correct's
// TALLY); the per-row counts are those of the final plane, not sums over passes.
// The plane is read by km_load_chunks and, where a chunk's other bytes are needed (its Ns at the start with FIXN, the chunk
// that is rewritten at the end unless FLAGS), the same 16 bytes once more, as km_correct reads them; nothing goes through
// global memory between passes.
// This kernel spells out the rule (stage D), its window loop (stage W), the counter flush and its LDS carving itself, statement
// for statement what km_decide and the helpers above say: the forms that went through them compiled to other instructions and
// those that were timed ran 0.8-1.2 % slower.  A change to the rule is made in km_decide AND in stage D here;
// tests/test_gpu_kmer_passes.py holds the two to each other (passes = 1 against km_correct, P passes against P launches).
constexpr int KM_MAX_PASSES = 8;

template <bool NIB, int FIXN = KM_FIXN_OFF, bool FLAGS = false, bool UNRES = false, bool TALLY = false>
__global__ __launch_bounds__(KM_THREADS) void km_correct_passes(KmerParams p, int passes, KmerTally q)
{
    static_assert(!FLAGS || (!NIB && FIXN == KM_FIXN_OFF), "the flag form: character rows, no N rule");
    static_assert(!UNRES || FLAGS, "unresolved bases are a value of the flag plane: the flag form only");
    static_assert(!TALLY || !FLAGS, "the tally plane goes with the corrected plane: the corrected form only");
    static_assert(KM_LDS_PASSES.chunk == 8 && KM_LDS_PASSES.row == 2 && KM_LDS_PASSES.wg == 1, "the carving below");
    extern __shared__ u32 km_lds[];
    const int E = p.rows_per_wg * p.cpr;
    u32* code0 = km_lds; u32* brk0 = km_lds + E;
    u32* cc = km_lds + 2 * E; u32* cb = km_lds + 3 * E;                  // r_(p-1)
    u32* nc = km_lds + 4 * E; u32* nb = km_lds + 5 * E;                  // r_p
    u32* sv = km_lds + 6 * E; u32* mark = km_lds + 7 * E;
    u32* nchg = km_lds + 8 * E;
    int* last = reinterpret_cast<int*>(nchg + p.rows_per_wg);
    int* wglast = last + p.rows_per_wg;
    const int64_t row0 = (int64_t)blockIdx.x * p.rows_per_wg;
    for (int i = threadIdx.x; i < p.rows_per_wg; i += KM_THREADS) { nchg[i] = 0; last[i] = -1; }
    if (threadIdx.x == 0) *wglast = -1;
    const int nr = km_load_chunks<NIB>(p, row0, code0, brk0);
    for (int e = threadIdx.x; e < nr * p.cpr; e += KM_THREADS) {          // the elements this thread loaded itself
        cc[e] = code0[e]; cb[e] = brk0[e]; mark[e] = 0;
        if constexpr (FIXN != KM_FIXN_OFF) {
            const int r = e / p.cpr, ch = e - r * p.cpr;
            u32 w[4];
            km_read_chunk<NIB>(p.seq + km_chunk_at<NIB>(p, row0 + r, ch), w);
            brk0[e] |= km_chunk_ns<NIB, FIXN>(p, w, brk0[e], row0 + r, ch) << 16;
        }
    }
    __syncthreads();
    const int k = p.k;
    const u64 kmask = (1ull << k) - 1;
    for (int pass = 0; pass < passes; ++pass) {
        // the window bits of r_(p-1): all of them in the first pass, then those over a base the pass before changed
        for (int e = threadIdx.x; e < nr * p.cpr; e += KM_THREADS) {
            const int r = e / p.cpr, ch = e - r * p.cpr;
            if (pass > 0 && last[r] < pass - 1) continue;                 // the row is finished
            u64 dirty = ~0ull;
            u32 valid = 0, solid = 0;
            if (pass > 0) {
                dirty = 0;
                for (int i = 0; i < 3; ++i)
                    if (ch + i < p.cpr) dirty |= (u64)(mark[e + i] & 0xFFFFu) << (16 * i);
                if (!dirty) continue;
                valid = sv[e] & 0xFFFFu; solid = sv[e] >> 16;
            }
            u64 b;
            const unsigned __int128 x = km_words(p, cc, cb, r * p.cpr, ch, 3, &b);
            for (int o = 0; o < 16; ++o) {
                if (!((dirty >> o) & kmask)) continue;
                valid &= ~(1u << o); solid &= ~(1u << o);
                if ((b >> o) & kmask) continue;
                valid |= 1u << o;
                if (km_solid(p, km_window(x, o, k))) solid |= 1u << o;
            }
            sv[e] = solid << 16 | valid;
        }
        __syncthreads();
        // trust and the two rules on r_(p-1); the decisions go to r_p
        for (int e = threadIdx.x; e < nr * p.cpr; e += KM_THREADS) {
            const int r = e / p.cpr, ch = e - r * p.cpr;
            if (pass > 0 && last[r] < pass - 1) continue;                 // (a row changed in this pass reads as `pass`: not finished)
            u64 V = 0, S = 0;                                             // bit i: the window starting at base 16 (ch - 2) + i
            for (int i = 0; i < 3; ++i) {
                const int c = ch - 2 + i;
                const u32 w = c >= 0 ? sv[r * p.cpr + c] : 0u;
                V |= (u64)(w & 0xFFFFu) << (16 * i);
                S |= (u64)(w >> 16) << (16 * i);
            }
            const u32 code_own = cc[e], brk_own = cb[e];
            u32 code_new = code_own, brk_new = brk_own, chg = 0, unres = 0;
            bool have_words = false;
            unsigned __int128 xa = 0, xb = 0;                            // chunks ch - 2 .. ch + 1 and ch .. ch + 3
            u32 ns = 0;                                                   // N rule: the Ns of the read that are still Ns
            if constexpr (FIXN != KM_FIXN_OFF) ns = (brk0[e] >> 16) & brk_own;
            for (int t = 0; t < 16; ++t) {
                if constexpr (FIXN != KM_FIXN_OFF) {
                    if ((ns >> t) & 1u) {
                        if (!have_words) {
                            u64 unused;
                            xa = km_words(p, cc, cb, r * p.cpr, ch - 2, 4, &unused);
                            xb = km_words(p, cc, cb, r * p.cpr, ch, 4, &unused);
                            have_words = true;
                        }
                        const unsigned __int128 B = km_breaks(p, cb, r * p.cpr, ch - 2, 5);   // bit i: base 16 (ch - 2) + i
                        const int pp = 32 + t;
                        int s[4] = {0, 0, 0, 0};
                        for (int j = pp - k + 1; j <= pp; ++j) {          // a candidate window: this N is its only break
                            if (((u64)(B >> j) & kmask) != 1ull << (pp - j)) continue;
                            const u64 f = j < 32 ? km_window(xa, j, k) : km_window(xb, j - 32, k);   // a break's code is 0
                            #pragma unroll
                            for (u32 x = 0; x < 4; ++x) s[x] += km_solid(p, f | (u64)x << (2 * (k - 1 - (pp - j)))) ? 1 : 0;
                        }
                        int best = -1, bs = 0; bool tie = false;
                        #pragma unroll
                        for (int x = 0; x < 4; ++x) {
                            if (s[x] > bs) { bs = s[x]; best = x; tie = false; }
                            else if (s[x] == bs && bs > 0) tie = true;
                        }
                        if (best < 0 || tie) continue;
                        code_new |= (u32)best << (30 - 2 * t);           // an ordinary base from the next pass on
                        brk_new &= ~(1u << t);
                        chg |= 1u << t;
                        continue;
                    }
                }
                if ((brk_own >> t) & 1u) continue;                        // a break: never changed
                const int pp = 32 + t;                                    // the base's index in the 48-bit window masks
                const u64 cover = kmask << (pp - k + 1);
                if ((S & cover) || !(V & cover)) continue;                // trusted
                if (!have_words) {
                    u64 unused;
                    xa = km_words(p, cc, cb, r * p.cpr, ch - 2, 4, &unused);
                    xb = km_words(p, cc, cb, r * p.cpr, ch, 4, &unused);
                    have_words = true;
                }
                const u32 orig = (code_own >> (30 - 2 * t)) & 3u;
                int s[4] = {0, 0, 0, 0};
                for (u32 alt = 0; alt < 4; ++alt) {
                    if (alt == orig) continue;
                    for (u64 m = V & cover; m; m &= m - 1) {
                        const int j = __builtin_ctzll(m);                 // a valid covering window
                        const u64 f = (j < 32 ? km_window(xa, j, k) : km_window(xb, j - 32, k)) ^ ((u64)(orig ^ alt) << (2 * (k - 1 - (pp - j))));
                        s[alt] += km_solid(p, f) ? 1 : 0;
                    }
                }
                int best = -1, bs = 0; bool tie = false;
                for (int alt = 0; alt < 4; ++alt) {
                    if (alt == (int)orig) continue;
                    if (s[alt] > bs) { bs = s[alt]; best = alt; tie = false; }
                    else if (s[alt] == bs && bs > 0) tie = true;
                }
                if (best < 0 || tie) {                                    // untrusted, and no substitution wins: unresolved
                    if constexpr (UNRES || TALLY) unres |= 1u << t;
                    continue;
                }
                code_new ^= (orig ^ (u32)best) << (30 - 2 * t);
                chg |= 1u << t;
            }
            nc[e] = code_new; nb[e] = brk_new; mark[e] = chg | unres << 16;
            if (chg) { last[r] = pass; *wglast = pass; }
        }
        __syncthreads();
        { u32* x = cc; cc = nc; nc = x; x = cb; cb = nb; nb = x; }
        if (*wglast != pass) break;                                       // uniform: written before the barrier, next after the one above
    }
    // store: km_put wherever r_P differs from r_0
    for (int e = threadIdx.x; e < nr * p.cpr; e += KM_THREADS) {
        const int r = e / p.cpr, ch = e - r * p.cpr;
        const size_t at = km_chunk_at<NIB>(p, row0 + r, ch);
        u32 w[4];                                                        // the chunk as read, or of the flag plane: all 0
        km_read_chunk<NIB, FLAGS>(p.seq + at, w);
        const u32 code_end = cc[e];
        const u32 dcode = code0[e] ^ code_end, dbrk = (brk0[e] ^ cb[e]) & 0xFFFFu, un = UNRES || TALLY ? mark[e] >> 16 : 0u;
        int changed = 0, unres = 0;
        u32 left = 0;                                                     // TALLY: bit t, base t is as read and unresolved
        if (dcode | dbrk | un) {
            for (int t = 0; t < 16; ++t) {
                if (((dcode >> (30 - 2 * t)) & 3u) | ((dbrk >> t) & 1u)) {
                    km_put<NIB, FLAGS>(w, t, (code_end >> (30 - 2 * t)) & 3u);
                    ++changed;
                } else if ((un >> t) & 1u) {
                    if constexpr (TALLY) left |= 1u << t;
                    else km_flag(w, t, 2u);
                    ++unres;
                }
            }
        }
        km_write_chunk<NIB>(p.out + at, w);
        if constexpr (TALLY) km_tally_chunk<NIB>(q, at, left);
        if (changed | unres) atomicAdd(&nchg[r], (u32)changed | (u32)unres << 16);
    }
    if (p.changed || p.unresolved) {
        __syncthreads();
        for (int i = threadIdx.x; i < nr; i += KM_THREADS) {
            if (p.changed) p.changed[row0 + i] = nchg[i] & 0xFFFFu;
            if (p.unresolved) p.unresolved[row0 + i] = nchg[i] >> 16;
        }
    }
}

// ---- ranks: partition, exchange and merge ----------------------------------------------------------------------------------
constexpr int KM_MAX_BUCKETS = 1024;  // owners of one select; the per-bucket counters live in LDS
constexpr int KM_SEL_QUADS = 4;       // 4-slot quads per thread and tile: a tile is KM_THREADS * 16 slots
constexpr int KM_CURSOR_STRIDE = 16;  // u64 words between two buckets' cursors: one 128-byte line each

__host__ __device__ __forceinline__ u32 km_owner(u64 key, u32 nbuckets)
{
    return (u32)(((km_hash(key ^ 0x9E3779B97F4A7C15ull) >> 32) * (u64)nbuckets) >> 32);
}

// The 16 slots of thread `tid` in tile `tile`: quads tile * KM_THREADS * KM_SEL_QUADS + j * KM_THREADS + tid, each read with
// two 16-byte loads of keys and one of counts.  tag[i] = bucket << 16 | rank within the tile's bucket for a kept slot, ~0 else.
// LDS: cnt[nbuckets] counts the kept slots of the tile per bucket (added to, not cleared here).
__device__ __forceinline__ void km_select_tile(const u64* keys, const u32* counts, u64 quads, u64 tile, u32 min_count,
                                               u32 nbuckets, u32* cnt, u64 (&key)[4 * KM_SEL_QUADS],
                                               u32 (&val)[4 * KM_SEL_QUADS], u32 (&tag)[4 * KM_SEL_QUADS])
{
    #pragma unroll
    for (int j = 0; j < KM_SEL_QUADS; ++j) {
        const u64 q = (tile * KM_SEL_QUADS + j) * KM_THREADS + threadIdx.x;
        ulonglong2 ka = make_ulonglong2(KM_EMPTY, KM_EMPTY), kb = ka;
        uint4 c = make_uint4(0, 0, 0, 0);
        if (q < quads) {
            ka = *reinterpret_cast<const ulonglong2*>(keys + 4 * q);
            kb = *reinterpret_cast<const ulonglong2*>(keys + 4 * q + 2);
            c = *reinterpret_cast<const uint4*>(counts + 4 * q);
        }
        key[4 * j] = ka.x; key[4 * j + 1] = ka.y; key[4 * j + 2] = kb.x; key[4 * j + 3] = kb.y;
        val[4 * j] = c.x; val[4 * j + 1] = c.y; val[4 * j + 2] = c.z; val[4 * j + 3] = c.w;
    }
    #pragma unroll
    for (int i = 0; i < 4 * KM_SEL_QUADS; ++i) {
        tag[i] = ~0u;
        if (key[i] == KM_EMPTY || val[i] < min_count) continue;
        const u32 b = nbuckets > 1 ? km_owner(key[i], nbuckets) : 0u;
        tag[i] = b << 16 | atomicAdd(cnt + b, 1u);
    }
}

// sizes[b] += kept slots of bucket b (sizes zeroed by the caller); one global add per non-empty bucket per workgroup
__global__ __launch_bounds__(KM_THREADS) void km_select_sizes(const u64* keys, const u32* counts, u64 slots, u32 min_count,
                                                              u32 nbuckets, u64* sizes)
{
    __shared__ u32 cnt[KM_MAX_BUCKETS];
    for (u32 i = threadIdx.x; i < nbuckets; i += KM_THREADS) cnt[i] = 0;
    __syncthreads();
    const u64 quads = slots / 4, tiles = (quads + KM_THREADS * KM_SEL_QUADS - 1) / (KM_THREADS * KM_SEL_QUADS);
    u64 key[4 * KM_SEL_QUADS]; u32 val[4 * KM_SEL_QUADS], tag[4 * KM_SEL_QUADS];
    for (u64 t = blockIdx.x; t < tiles; t += gridDim.x)
        km_select_tile(keys, counts, quads, t, min_count, nbuckets, cnt, key, val, tag);
    __syncthreads();
    for (u32 i = threadIdx.x; i < nbuckets; i += KM_THREADS)
        if (cnt[i]) atomicAdd(sizes + i, (u64)cnt[i]);
}

// The kept slots of bucket b go to out_keys / out_counts [cursor[b * KM_CURSOR_STRIDE], ...): per tile, one returning add per
// non-empty bucket reserves the tile's run and every kept slot writes at run + its rank.  Order inside a bucket varies.
__global__ __launch_bounds__(KM_THREADS) void km_select_scatter(const u64* keys, const u32* counts, u64 slots, u32 min_count,
                                                                u32 nbuckets, u64* cursor, u64* out_keys, u32* out_counts)
{
    __shared__ u32 cnt[KM_MAX_BUCKETS];
    __shared__ u64 base[KM_MAX_BUCKETS];
    const u64 quads = slots / 4, tiles = (quads + KM_THREADS * KM_SEL_QUADS - 1) / (KM_THREADS * KM_SEL_QUADS);
    u64 key[4 * KM_SEL_QUADS]; u32 val[4 * KM_SEL_QUADS], tag[4 * KM_SEL_QUADS];
    for (u64 t = blockIdx.x; t < tiles; t += gridDim.x) {
        for (u32 i = threadIdx.x; i < nbuckets; i += KM_THREADS) cnt[i] = 0;
        __syncthreads();
        km_select_tile(keys, counts, quads, t, min_count, nbuckets, cnt, key, val, tag);
        __syncthreads();
        for (u32 i = threadIdx.x; i < nbuckets; i += KM_THREADS)
            if (cnt[i]) base[i] = atomicAdd(cursor + (size_t)i * KM_CURSOR_STRIDE, (u64)cnt[i]);
        __syncthreads();
        #pragma unroll
        for (int i = 0; i < 4 * KM_SEL_QUADS; ++i) {
            if (tag[i] == ~0u) continue;
            const u64 at = base[tag[i] >> 16] + (tag[i] & 0xFFFFu);
            out_keys[at] = key[i];
            out_counts[at] = val[i];
        }
        __syncthreads();                                              // base and cnt are reused by the next tile
    }
}

// counts[key] += c for n (key, count) pairs, the table as km_count's; a pair that finds neither its key nor an empty slot sets
// ST_KMER to its index (the lowest such) and a workgroup that starts a stride with the word set stops
__global__ __launch_bounds__(KM_THREADS) void km_merge(const u64* in_keys, const u32* in_counts, int64_t n, u64* keys, u32* counts,
                                                       u64 mask, u64* status)
{
    const int64_t stride = (int64_t)gridDim.x * KM_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * KM_THREADS + threadIdx.x; i < n; i += stride) {
        if (__hip_atomic_load(status + ST_KMER, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != ~0ull) return;
        if (!km_insert(keys, counts, mask, in_keys[i], in_counts[i])) { atomicMin(status + ST_KMER, (u64)i); return; }
    }
}

// ---- partitions: the count split in time on one GPU (kbbq correct --partitions; kbbq/kmer.py count_partitioned) --------------
// part(key, P) = km_owner(key, P), the split the ranks use in space.  Round p of P counts, over all rows, exactly the windows
// whose canonical key has part == p, into a table 1 / P the size: a key lies in one partition, so its count there is its
// global count, and the rounds' histograms add up to the one table's.  The two kernels are km_count / km_count_filtered with one
// test in front of the insert -- in the filtered form in front of the load of twice[word] too, so a round reads the filter
// for its own keys alone.  The grid, the LDS plan (KM_LDS_COUNT), the rows per workgroup and the walk are km_count's; every
// round hashes every window (canonical key, one mix for the owner), which is what P rounds cost beside one.
struct KmerPartParams { u32 parts, part; };   // 1 <= parts <= KM_MAX_BUCKETS, part < parts

template <bool NIB>
__global__ __launch_bounds__(KM_THREADS) void km_count_part(KmerParams p, KmerPartParams q)
{
    extern __shared__ u32 km_lds[];
    u32* code = km_lds_chunk(km_lds, p, 0); u32* brk = km_lds_chunk(km_lds, p, 1);
    const int64_t row0 = (int64_t)blockIdx.x * p.rows_per_wg;
    const int nr = km_load_chunks<NIB>(p, row0, code, brk);
    __syncthreads();
    if (km_table_full(p)) return;
    km_walk(p, code, brk, nr, [&](int r, int, int, u64 f) {
        const u64 key = km_canonical(f, p.k);
        if (km_owner(key, q.parts) != q.part) return true;                // another round's key
        if (km_insert(p.keys, p.counts, p.mask, key, 1u)) return true;
        atomicMin(p.status + ST_KMER, (u64)(row0 + r));
        return false;
    });
}

template <bool NIB>
__global__ __launch_bounds__(KM_THREADS) void km_count_filtered_part(KmerParams p, KmerFilterParams f, KmerPartParams q)
{
    extern __shared__ u32 km_lds[];
    u32* code = km_lds_chunk(km_lds, p, 0); u32* brk = km_lds_chunk(km_lds, p, 1);
    const int64_t row0 = (int64_t)blockIdx.x * p.rows_per_wg;
    const int nr = km_load_chunks<NIB>(p, row0, code, brk);
    __syncthreads();
    if (km_table_full(p)) return;
    km_walk(p, code, brk, nr, [&](int r, int, int, u64 fw) {
        const u64 key = km_canonical(fw, p.k);
        if (km_owner(key, q.parts) != q.part) return true;                // another round's key: its filter word is not read
        u64 m;
        const u64 w = km_filter_index(key, f.wmask, &m);
        if ((f.twice[w] & m) != m) return true;                           // seen once
        if (km_insert(p.keys, p.counts, p.mask, key, 1u)) return true;
        atomicMin(p.status + ST_KMER, (u64)(row0 + r));
        return false;
    });
}

// ---- quality gate: count only the windows of bases with quality >= Q (kbbq correct --kmer-min-qual; kbbq/kmer.py gate_plane) ----
// A base is countable when it is A/C/G/T and its quality byte is >= qual_byte_min; a window is counted iff all k of its bases
// are.  The gate only changes which positions are breaks, so it is a pre-pass: km_gate writes a copy of the sequence plane with
// 'N' (4-bit planes: code 4) wherever the quality byte is below qual_byte_min -- every other byte as read, every byte of every
// row written, padding and separator included -- and km_prefilter, km_count, km_count_filtered and the _part forms read that
// copy unchanged.  Nothing after the count reads it: the correction kernels run on the rows as read.
// Work split: km_count's.  A thread loads its chunk once (km_read_chunk) and the 16 quality bytes beside it (quality planes are
// [nrows, 16 cpr] characters, at twice the chunk's offset beside nibbles, as km_tally_chunk's), stores the gated chunk
// (km_write_chunk) and puts the chunk's break mask -- km_load_chunks' mask of the gated bases -- into LDS.  After the barrier it
// counts the window starts of its chunk that see no break in k bases, km_chunk_windows' test on the masks of its chunk and the
// next two; the sums meet in one LDS word and every workgroup makes one 64-bit add to *windows (NULL: no count).  Counting
// `out` with any count kernel inserts exactly that many windows.
struct KmerGate { const uint8_t* qual; u32 qual_byte_min; uint8_t* out; u64* windows; };
constexpr KmLds KM_LDS_GATE = {1, 0, 1};        // km_gate: brk; the workgroup's windows

template <bool NIB>
__global__ __launch_bounds__(KM_THREADS) void km_gate(KmerParams p, KmerGate g)
{
    extern __shared__ u32 km_lds[];
    u32* brk = km_lds_chunk(km_lds, p, 0);
    u32* sum = km_lds_wg(km_lds, KM_LDS_GATE, p);
    const int64_t row0 = (int64_t)blockIdx.x * p.rows_per_wg;
    const int nr = (int)(p.nrows - row0 < p.rows_per_wg ? p.nrows - row0 : p.rows_per_wg);
    if (threadIdx.x == 0) *sum = 0;
    for (int e = threadIdx.x; e < nr * p.cpr; e += KM_THREADS) {
        const int r = e / p.cpr, ch = e - r * p.cpr;
        const int64_t row = row0 + r;
        const int L = (int)(p.meta[row] & 0xFFFFu);
        const size_t at = km_chunk_at<NIB>(p, row, ch);
        u32 w[4];
        km_read_chunk<NIB>(p.seq + at, w);
        const uint4 qv = *reinterpret_cast<const uint4*>(g.qual + (NIB ? 2 * at : at));
        const u32 q[4] = {qv.x, qv.y, qv.z, qv.w};
        u32 b = 0;
        #pragma unroll
        for (int t = 0; t < 16; ++t) {
            const bool low = ((q[t >> 2] >> (8 * (t & 3))) & 0xFFu) < g.qual_byte_min;
            bool base;
            if constexpr (NIB) {
                const int sh = km_nib_shift(t & 7);
                if (low) w[t >> 3] = (w[t >> 3] & ~(0xFu << sh)) | (4u << sh);
                base = ((w[t >> 3] >> sh) & 0xFu) < 4u;
            } else {
                const int sh = 8 * (t & 3);
                if (low) w[t >> 2] = (w[t >> 2] & ~(0xFFu << sh)) | ((u32)'N' << sh);
                const u32 x = (w[t >> 2] >> sh) & 0xFFu;
                base = x == 'A' || x == 'C' || x == 'G' || x == 'T';
            }
            b |= (base && ch * 16 + t < L ? 0u : 1u) << t;
        }
        km_write_chunk<NIB>(g.out + at, w);
        brk[e] = b;
    }
    if (!g.windows) return;                                               // uniform: a kernel parameter
    __syncthreads();
    const u64 kmask = (1ull << p.k) - 1;
    u32 mine = 0;
    for (int e = threadIdx.x; e < nr * p.cpr; e += KM_THREADS) {
        const int r = e / p.cpr, ch = e - r * p.cpr;
        // the masks of chunks ch .. ch + 2, past the row all breaks: km_breaks' words, spelled out here because a third caller of
        // km_breaks moved a register in the N-rule forms of km_correct_passes, and no existing kernel is to change
        u64 m = 0;
        for (int i = 0; i < 3; ++i) m |= (u64)(ch + i < p.cpr ? brk[e + i] : 0xFFFFu) << (16 * i);
        for (int o = 0; o < 16; ++o) mine += ((m >> o) & kmask) ? 0u : 1u;
    }
    if (mine) atomicAdd(sum, mine);
    __syncthreads();
    if (threadIdx.x == 0 && *sum) atomicAdd(g.windows, (u64)*sum);
}
