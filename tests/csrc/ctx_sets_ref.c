/* Test reference for include/cabac_hip_ctx_sets.h: orc_encode_records / orc_decode_records of the oracle started from given
 * contexts, the contexts they leave copied out.  The oracle itself is included unchanged and its own static coder is used
 * (ctx_store, enc_start / encode_record_run / finish_stream, dec_start / dec_bin / ... / dec_finish): nothing is restated here
 * but the two drivers.  Built by tests/ctx_sets_model.py with plain cc. */
#include "../../oracle/cabac_oracle.c"

static void store_from(ctx_store *c, const uint16_t *s0, const uint16_t *s1, const uint8_t *rate) {
  memcpy(c->s0, s0, sizeof c->s0);
  memcpy(c->s1, s1, sizeof c->s1);
  memcpy(c->rate, rate, sizeof c->rate);
}

static void store_to(const ctx_store *c, uint16_t *s0, uint16_t *s1, uint8_t *rate) {
  memcpy(s0, c->s0, sizeof c->s0);
  memcpy(s1, c->s1, sizeof c->s1);
  memcpy(rate, c->rate, sizeof c->rate);
}

/* orc_encode_records from (s0, s1, rate) instead of ctx_store_init; the contexts after the last record -> (o0, o1, orate).
 * Return value and n_bits as orc_encode_records. */
long csr_encode_records_from(const uint16_t *rec, long n, const uint16_t *s0, const uint16_t *s1, const uint8_t *rate, int flags,
                             uint8_t *out, long cap, uint32_t *n_bits, uint16_t *o0, uint16_t *o1, uint8_t *orate) {
  bit_sink s = {out, cap, 0, 0, 0, 0};
  bin_enc e;
  e.out = &s;
  store_from(&e.ctx, s0, s1, rate);
  enc_start(&e);
  if (encode_record_run(&e, rec, n)) return -2;
  store_to(&e.ctx, o0, o1, orate);
  return finish_stream(&e, &s, flags, n_bits);
}

/* orc_decode_records from (s0, s1, rate); return value, bins and n_bits_read as orc_decode_records */
int csr_decode_records_from(const uint16_t *rec, long n, const uint16_t *s0, const uint16_t *s1, const uint8_t *rate, int flags,
                            const uint8_t *in, long n_in, uint8_t *bins, uint32_t *n_bits_read, uint16_t *o0, uint16_t *o1,
                            uint8_t *orate) {
  bin_dec d;
  memset(&d, 0, sizeof d);
  d.in = in;
  d.n_in = n_in;
  store_from(&d.ctx, s0, s1, rate);
  dec_start(&d);
  for (long i = 0; i < n; i++) {
    unsigned id = rec[i] & CABAC_REC_ID_MASK;
    if (id < ORC_NUM_CTX) bins[i] = (uint8_t)dec_bin(&d, id);
    else if (id == CABAC_REC_EP) bins[i] = (uint8_t)dec_ep(&d);
    else if (id == CABAC_REC_TRM) bins[i] = (uint8_t)dec_trm(&d);
    else if (id == CABAC_REC_ALIGN) { d.range = 256; bins[i] = 0; }
    else return -2;
    if (d.underrun) return -4;
  }
  if (n_bits_read) *n_bits_read = (uint32_t)(8 * d.idx + d.bits_needed);
  if (d.underrun) return -4;
  store_to(&d.ctx, o0, o1, orate);
  if (flags & 1) return dec_finish(&d);
  return 0;
}
