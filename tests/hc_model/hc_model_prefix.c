/*
 * tests/hc_model/hc_model_prefix.c -- CPU model of the HC parse of a block
 * with a prefix (lz4m_compress_hc_dict_batch, python-lz4_amd/csrc/lz4m_hc.hip),
 * as DESIGN.md section 9.5 defines it.  The HIP kernel must produce these
 * bytes.  Plain C99; it builds on the tables, the search and the sequence
 * writer of hc_model.c, which it includes (so this file alone is the
 * translation unit, and hc_model_compress / hc_model_decode come with it).
 *
 * The block is the n bytes at base + prefix_len; the prefix_len (0..65536)
 * bytes before it are its history.  Positions count from `base`:
 *   insert    before the parse starts at ip = anchor = prefix_len, every
 *             prefix position is in the tables (each has four readable bytes
 *             when a parse takes place at all, n >= 13); afterwards, as in
 *             section 9.1, every position below a search position is;
 *   search    unchanged: a candidate may lie anywhere at or above 0, its
 *             backward extension stops at position 0; low >= anchor >=
 *             prefix_len, so no emitted match starts in the prefix and no
 *             literal comes from it;
 *   end       the rules apply to the block: no match starts after prefix_len
 *             + n - 12, none extends past prefix_len + n - 5, blocks below 13
 *             bytes are one literal run, n = 0 gives the block 00;
 *   output    limited as in section 9.1.
 * With prefix_len = 0 the bytes are hc_model_compress's.
 */
#include "hc_model.c"

int hc_model_compress_prefix(const uint8_t* base, int prefix_len, int n, uint8_t* dst, int cap, int level) {
    if (n < 0 || cap < 0 || n > 0x7E000000 || prefix_len < 0 || prefix_len > 65536) return 0;
    hc_state s;
    const int32_t P = prefix_len, total = P + n;
    s.src = base;
    s.n = total;
    s.inserted = 0;
    s.attempts = hc_model_attempts(level);
    s.head = (uint32_t*)calloc((size_t)1 << HC_HASH_BITS, sizeof(uint32_t));
    s.chain = (uint16_t*)calloc(65536, sizeof(uint16_t));
    if (!s.head || !s.chain) {
        free(s.head);
        free(s.chain);
        return 0;
    }
    int64_t op = 0;   /* bytes produced */
    int32_t anchor = P, ip = P;
    int fits = 1;
    const int32_t mflimit = total - 12;
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
                if (!hc_emit(base, anchor, start - anchor, start - mpos, s2 - start, dst, &op, cap)) {
                    fits = 0;
                    break;
                }
                anchor = s2;
            }
            start = s2;
            ml = m2;
            mpos = p2;
        }
        if (!fits || !hc_emit(base, anchor, start - anchor, start - mpos, ml, dst, &op, cap)) {
            fits = 0;
            break;
        }
        ip = start + ml;
        anchor = ip;
    }
    if (fits) {
        const int32_t ll = total - anchor;
        const int64_t need = 1 + (int64_t)ext_bytes(ll) + ll;
        if (op + need > cap) {
            fits = 0;
        } else {
            uint8_t* o = dst + op;
            *o++ = (uint8_t)((ll < 15 ? ll : 15) << 4);
            o = put_ext(o, ll);
            if (ll) memcpy(o, base + anchor, (size_t)ll);
            op += need;
        }
    }
    free(s.head);
    free(s.chain);
    return fits ? (int)op : 0;
}

/* hc_model_decode with a dictionary: the block's history is the dict_len
 * bytes at dict; returns the decoded size or -1 */
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
