/*
 * tests/hc_model/hc_model.c -- CPU model of the hash-chain ("HC") LZ4 block
 * parse of lz4m_compress_hc_batch and, with a prefix, of
 * lz4m_compress_hc_dict_batch (python-lz4_amd/csrc/lz4m_hc.hip), as DESIGN.md
 * sections 9.1 and 9.5 define it.  The HIP kernels must produce these bytes.
 * Its tables, level table, sequence writer and decoder are also those of the
 * optimal parse's model (opt_model.c, which includes this file).  Plain C99,
 * no dependency; the tests build it with gcc at run time.
 *
 * The parse, serially:
 *   hash      h(p) = (LE32(src + p) * 2654435761) >> (32 - 13); head[h] is the
 *             newest inserted position with that hash, chain[p mod 65536] the
 *             distance from p to the previous position with p's hash (0: none,
 *             or further than 65535 bytes away);
 *   insert    before a search at position ip, every position below ip is in
 *             the tables;
 *   search    search(q, low): walk the chain from head[h(q)], newest first,
 *             while the candidate is at most 65535 bytes back, for at most
 *             `attempts` candidates; a candidate c with >= 4 common bytes
 *             forwards (at most n - 5 - q) also grows backwards over equal
 *             bytes while its start stays >= low and c's stays >= 0; keep the
 *             longest (backward + forward), the first (nearest) among equals;
 *   parse     at ip (literals pending since `anchor`): M = search(ip, anchor);
 *             none: ip + 1.  Else probe the end of M: q = start(M) + len(M)
 *             - 2; while q <= n - 12: M2 = search(q, start(M)); if M2 is not
 *             longer than M stop; else if M2 starts >= 4 bytes after M, M is
 *             cut to end where M2 starts and is emitted, otherwise M is
 *             dropped; M = M2 and the probe repeats.  Emit M, ip = end(M);
 *   end       no match starts after n - 12, none extends past n - 5, blocks
 *             below 13 bytes are literals only (lz4.c MFLIMIT / LASTLITERALS);
 *   output    the block is written only if all of it fits in `cap` bytes;
 *             otherwise the result is 0 and nothing past dst + cap is touched.
 *
 * With a prefix (hc_model_compress_prefix) the block is the n bytes at base +
 * prefix_len; the prefix_len (0..65536) bytes before it are its history.
 * Positions count from `base`:
 *   insert    before the parse starts at ip = anchor = prefix_len, every
 *             prefix position is in the tables (each has four readable bytes
 *             when a parse takes place at all, n >= 13); afterwards, as above,
 *             every position below a search position is;
 *   search    unchanged: a candidate may lie anywhere at or above 0, its
 *             backward extension stops at position 0; low >= anchor >=
 *             prefix_len, so no emitted match starts in the prefix and no
 *             literal comes from it;
 *   end       the rules apply to the block: no match starts after prefix_len
 *             + n - 12, none extends past prefix_len + n - 5, blocks below 13
 *             bytes are one literal run, n = 0 gives the block 00;
 *   output    limited as above.
 * hc_model_compress is this parse with prefix_len = 0.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define HC_HASH_BITS 13
#define HC_MAX_DIST 65535
#define HC_MAX_INPUT 0x7E000000

int hc_model_attempts(int level) {
    if (level < 1) level = 9;          /* lz4hc.c: cLevel < 1 -> LZ4HC_CLEVEL_DEFAULT */
    if (level > 9) level = 9;          /* deeper searches for levels 10-12 are not modelled */
    return level < 3 ? 2 : 1 << (level - 1);   /* lz4hc.c level table: 3 -> 4 ... 9 -> 256 */
}

static uint32_t le32(const uint8_t* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

static uint32_t hc_hash(const uint8_t* p) { return (le32(p) * 2654435761u) >> (32 - HC_HASH_BITS); }

typedef struct {
    const uint8_t* src;
    int32_t n;
    uint32_t* head;    /* position + 1, 0 = empty */
    uint16_t* chain;
    int32_t inserted;  /* positions below this one are in the tables */
    int attempts;
} hc_state;

/* empty tables over the n bytes at src; 0 if there is no memory for them */
static int hc_open(hc_state* s, const uint8_t* src, int32_t n, int level) {
    s->src = src;
    s->n = n;
    s->inserted = 0;
    s->attempts = hc_model_attempts(level);
    s->head = (uint32_t*)calloc((size_t)1 << HC_HASH_BITS, sizeof(uint32_t));
    s->chain = (uint16_t*)calloc(65536, sizeof(uint16_t));
    return s->head && s->chain;
}

static void hc_close(hc_state* s) {
    free(s->head);
    free(s->chain);
}

static void hc_insert_to(hc_state* s, int32_t end) {
    for (int32_t p = s->inserted; p < end; ++p) {
        const uint32_t h = hc_hash(s->src + p);
        const uint32_t prev = s->head[h];
        const uint32_t d = prev ? (uint32_t)p + 1u - prev : 0u;
        s->chain[p & 0xFFFF] = (uint16_t)(d > HC_MAX_DIST ? 0u : d);
        s->head[h] = (uint32_t)p + 1u;
    }
    if (end > s->inserted) s->inserted = end;
}

/* search(q, low), every position below q inserted: returns the longest
 * match's length (0: none) with its start in *start (low <= *start <= q) and
 * the start of its source in *pos */
static int32_t hc_search(hc_state* s, int32_t q, int32_t low, int32_t* start, int32_t* pos) {
    const uint8_t* src = s->src;
    const int32_t lim = s->n - 5 - q;
    int32_t best = 0;
    uint32_t cur = s->head[hc_hash(src + q)];
    for (int left = s->attempts; left > 0 && cur != 0 && q - (int32_t)(cur - 1) <= HC_MAX_DIST; --left) {
        const int32_t c = (int32_t)(cur - 1);
        int32_t fwd = 0;
        while (fwd < lim && src[c + fwd] == src[q + fwd]) ++fwd;
        if (fwd >= 4) {
            int32_t back = 0;
            while (q - back > low && c - back > 0 && src[q - back - 1] == src[c - back - 1]) ++back;
            if (fwd + back > best) {
                best = fwd + back;
                *start = q - back;
                *pos = c - back;
                if (best == lim + q - low) break;   /* nothing longer exists */
            }
        }
        const uint32_t d = s->chain[c & 0xFFFF];
        cur = d ? cur - d : 0;
    }
    return best;
}

static int32_t ext_bytes(int32_t v) { return v >= 15 ? 1 + (v - 15) / 255 : 0; }

static uint8_t* put_ext(uint8_t* op, int32_t v) {
    if (v >= 15) {
        v -= 15;
        for (; v >= 255; v -= 255) *op++ = 255;
        *op++ = (uint8_t)v;
    }
    return op;
}

/* one sequence at dst + *op if it fits in cap: ll literals from lits, then
 * (ml > 0) a match of ml bytes at distance off; ml == 0 is the block's last
 * sequence, its literal run alone */
static int hc_emit(const uint8_t* lits, int32_t ll, int32_t off, int32_t ml, uint8_t* dst, int64_t* op, int cap) {
    const int64_t need = 1 + (int64_t)ext_bytes(ll) + ll + (ml ? 2 + ext_bytes(ml - 4) : 0);
    if (*op + need > cap) return 0;
    uint8_t* o = dst + *op;
    *o++ = (uint8_t)(((ll < 15 ? ll : 15) << 4) | (ml ? (ml - 4 < 15 ? ml - 4 : 15) : 0));
    o = put_ext(o, ll);
    if (ll) memcpy(o, lits, (size_t)ll);
    o += ll;
    if (ml) {
        *o++ = (uint8_t)(off & 0xFF);
        *o++ = (uint8_t)(off >> 8);
        o = put_ext(o, ml - 4);
    }
    *op += need;
    return 1;
}

/* the parse of the n bytes at base + P with the P bytes before them as history */
static int hc_parse(const uint8_t* base, int32_t P, int32_t n, uint8_t* dst, int cap, int level) {
    if (n < 0 || cap < 0 || n > HC_MAX_INPUT || P < 0 || P > 65536) return 0;
    hc_state s;
    const int32_t total = P + n, mflimit = total - 12;
    if (!hc_open(&s, base, total, level)) {
        hc_close(&s);
        return 0;
    }
    int64_t op = 0;   /* bytes produced */
    int32_t anchor = P, ip = P;
    int fits = 1;
    if (n >= 13) hc_insert_to(&s, P);   /* the prefix */
    while (n >= 13 && ip <= mflimit) {
        int32_t start = 0, mpos = 0, ml;
        hc_insert_to(&s, ip);
        ml = hc_search(&s, ip, anchor, &start, &mpos);
        if (ml == 0) {
            ++ip;
            continue;
        }
        for (;;) {   /* probe the end of the match for a longer one that overlaps it */
            const int32_t q = start + ml - 2;
            int32_t s2 = 0, p2 = 0, m2;
            if (q > mflimit) break;
            hc_insert_to(&s, q);
            m2 = hc_search(&s, q, start, &s2, &p2);
            if (m2 <= ml) break;
            if (s2 - start >= 4) {   /* keep the head of the first match */
                if (!hc_emit(base + anchor, start - anchor, start - mpos, s2 - start, dst, &op, cap)) {
                    fits = 0;
                    break;
                }
                anchor = s2;
            }
            start = s2;
            ml = m2;
            mpos = p2;
        }
        if (!fits || !hc_emit(base + anchor, start - anchor, start - mpos, ml, dst, &op, cap)) {
            fits = 0;
            break;
        }
        ip = start + ml;
        anchor = ip;
    }
    if (fits) fits = hc_emit(base + anchor, total - anchor, 0, 0, dst, &op, cap);
    hc_close(&s);
    return fits ? (int)op : 0;
}

int hc_model_compress(const uint8_t* src, int n, uint8_t* dst, int cap, int level) {
    return hc_parse(src, 0, n, dst, cap, level);
}

int hc_model_compress_prefix(const uint8_t* base, int prefix_len, int n, uint8_t* dst, int cap, int level) {
    return hc_parse(base, prefix_len, n, dst, cap, level);
}

/* A small safe decoder (the check program decodes the models' output with
 * it): the block's history is the dict_len bytes at dict; returns the decoded
 * size, or -1 on any malformed or overlong input. */
int hc_model_decode_prefix(const uint8_t* src, int n, const uint8_t* dict, int dict_len, uint8_t* dst, int cap) {
    int64_t ip = 0, op = 0;
    if (n <= 0 || dict_len < 0) return -1;
    for (;;) {
        if (ip >= n) return -1;
        const uint32_t tok = src[ip++];
        int64_t ll = tok >> 4;
        if (ll == 15) {
            uint32_t b;
            do {
                if (ip >= n) return -1;
                b = src[ip++];
                ll += b;
            } while (b == 255);
        }
        if (ll > n - ip || ll > cap - op) return -1;
        if (ll) memcpy(dst + op, src + ip, (size_t)ll);
        ip += ll;
        op += ll;
        if (ip == n) return (tok & 15) ? -1 : (int)op;
        if (n - ip < 2) return -1;
        const int64_t off = (int64_t)src[ip] | ((int64_t)src[ip + 1] << 8);
        ip += 2;
        int64_t ml = tok & 15;
        if (ml == 15) {
            uint32_t b;
            do {
                if (ip >= n) return -1;
                b = src[ip++];
                ml += b;
            } while (b == 255);
        }
        ml += 4;
        if (off == 0 || off > op + dict_len || ml > cap - op) return -1;
        for (int64_t k = 0; k < ml; ++k) {
            const int64_t from = op + k - off;
            dst[op + k] = from >= 0 ? dst[from] : dict[dict_len + from];
        }
        op += ml;
    }
}

int hc_model_decode(const uint8_t* src, int n, uint8_t* dst, int cap) {
    return hc_model_decode_prefix(src, n, NULL, 0, dst, cap);
}
