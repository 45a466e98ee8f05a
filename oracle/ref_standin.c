/* ref_standin.c — TEST INFRASTRUCTURE ONLY: the 11 htslib symbols the reference (haowenz/FEM v0.2) links against, as a
 * plain text-SAM writer written from the SAM v1 specification (sections 1.3-1.5 for the text, 4.2 for the record
 * layout the reference fills in src/align.c:546-632).  Declarations: oracle/ref_standin/htslib/sam.h.  With these two
 * files the reference's sources compile and link from where they lie (`make -C oracle ref`), so that the tests can
 * compare the oracle and the kernels with what the reference itself computes.  htslib's own rendering stays unpinned:
 * a field this writer prints is what the reference PUT INTO the record, printed by the specification's rules.
 */
#include <stdlib.h>
#include <string.h>

#include "htslib/sam.h"

const unsigned char seq_nt16_table[256] = {
    15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
    15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
    15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
    15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,  0, 15, 15,
    15,  1, 14,  2, 13, 15, 15,  4, 11, 15, 15, 12, 15,  3, 15, 15,
    15, 15,  5,  6,  8, 15,  7,  9, 15, 10, 15, 15, 15, 15, 15, 15,
    15,  1, 14,  2, 13, 15, 15,  4, 11, 15, 15, 12, 15,  3, 15, 15,
    15, 15,  5,  6,  8, 15,  7,  9, 15, 10, 15, 15, 15, 15, 15, 15,
    15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
    15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
    15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
    15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
    15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
    15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
    15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
    15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15};

bam1_t *bam_init1(void) { return (bam1_t *)calloc(1, sizeof(bam1_t)); }

void bam_destroy1(bam1_t *b) {
  if (!b) return;
  free(b->data);
  free(b);
}

/* Size of the value of an aux field of this type at p (BAM 4.2.4), or -1. */
static int aux_value_size(const uint8_t *p, const uint8_t *end) {
  switch (*p) {
    case 'A': case 'c': case 'C': return 1;
    case 's': case 'S': return 2;
    case 'i': case 'I': case 'f': return 4;
    case 'Z': case 'H': {
      const uint8_t *q = p + 1;
      while (q < end && *q) ++q;
      return q < end ? (int)(q - p) : -1; /* characters + NUL, without the type byte */
    }
    default: return -1;
  }
}

/* Removes the field `tag` if the record has it, then appends tag + type + value. */
static int aux_put(bam1_t *b, const char tag[2], char type, const void *value, int n) {
  uint8_t *aux = bam_get_aux(b), *end = b->data + b->l_data, *p = aux;
  while (p + 3 <= end) {
    int sz = aux_value_size(p + 2, end);
    if (sz < 0) return -1;
    if (p[0] == (uint8_t)tag[0] && p[1] == (uint8_t)tag[1]) {
      memmove(p, p + 3 + sz, (size_t)(end - (p + 3 + sz)));
      b->l_data -= 3 + sz;
      break;
    }
    p += 3 + sz;
  }
  uint32_t need = (uint32_t)b->l_data + 3 + (uint32_t)n;
  if (need > b->m_data) {
    uint8_t *d = (uint8_t *)realloc(b->data, need);
    if (!d) return -1;
    b->data = d, b->m_data = need;
  }
  uint8_t *w = b->data + b->l_data;
  w[0] = (uint8_t)tag[0], w[1] = (uint8_t)tag[1], w[2] = (uint8_t)type;
  memcpy(w + 3, value, (size_t)n);
  b->l_data += 3 + n;
  return 0;
}

/* An integer in the smallest type that holds it (BAM 4.2.4: c C s S i I, little-endian). */
int bam_aux_update_int(bam1_t *b, const char tag[2], int64_t val) {
  uint8_t v[4];
  char type;
  int n;
  if (val < INT32_MIN || val > UINT32_MAX) return -1;
  if (val < 0) type = val >= INT8_MIN ? 'c' : val >= INT16_MIN ? 's' : 'i';
  else type = val <= UINT8_MAX ? 'C' : val <= UINT16_MAX ? 'S' : 'I';
  n = type == 'c' || type == 'C' ? 1 : type == 's' || type == 'S' ? 2 : 4;
  uint32_t u = (uint32_t)val;
  for (int i = 0; i < n; ++i) v[i] = (uint8_t)(u >> (8 * i));
  return aux_put(b, tag, type, v, n);
}

/* len counts the terminating NUL when the string has one at data[len - 1]; one is stored either way. */
int bam_aux_update_str(bam1_t *b, const char tag[2], int len, const char *data) {
  if (len < 0) len = (int)strlen(data) + 1;
  int n = len > 0 && data[len - 1] == '\0' ? len - 1 : len;
  char *z = (char *)malloc((size_t)n + 1);
  if (!z) return -1;
  memcpy(z, data, (size_t)n);
  z[n] = '\0';
  int rc = aux_put(b, tag, 'Z', z, n + 1);
  free(z);
  return rc;
}

samFile *sam_open_format(const char *path, const char *mode, const void *format) {
  (void)format;
  FILE *f = strcmp(path, "-") == 0 ? stdout : fopen(path, mode);
  if (!f) return NULL;
  samFile *s = (samFile *)calloc(1, sizeof(samFile));
  s->fp = f;
  return s;
}

int sam_close(samFile *s) {
  if (!s) return -1;
  int rc = s->fp == stdout ? fflush(stdout) : fclose(s->fp);
  free(s);
  return rc ? -1 : 0;
}

sam_hdr_t *sam_hdr_init(void) { return (sam_hdr_t *)calloc(1, sizeof(sam_hdr_t)); }

/* Frees what the header owns: the names still in target_name[] (the reference clears the ones it borrowed,
 * src/output_queue.c:38-40), the two arrays and the text. */
void sam_hdr_destroy(sam_hdr_t *h) {
  if (!h) return;
  if (h->target_name)
    for (int32_t i = 0; i < h->n_targets; ++i) free(h->target_name[i]);
  free(h->target_name);
  free(h->target_len);
  free(h->text);
  free(h);
}

int sam_hdr_write(samFile *s, const sam_hdr_t *h) {
  if (!s || !h) return -1;
  if (h->l_text && fwrite(h->text, 1, h->l_text, s->fp) != h->l_text) return -1;
  return 0;
}

/* One alignment line, SAMv1 1.4: the 11 mandatory fields, then the optional fields as TAG:TYPE:VALUE. */
int sam_write1(samFile *s, const sam_hdr_t *h, const bam1_t *b) {
  FILE *f = s->fp;
  const bam1_core_t *c = &b->core;
  fputs(c->l_qname > 0 && bam_get_qname(b)[0] ? bam_get_qname(b) : "*", f);
  fprintf(f, "\t%u\t", (unsigned)c->flag);
  if (c->tid >= 0 && c->tid < h->n_targets) fputs(h->target_name[c->tid], f);
  else fputc('*', f);
  fprintf(f, "\t%" PRId64 "\t%u\t", c->pos + 1, (unsigned)c->qual);
  if (c->n_cigar == 0) fputc('*', f);
  for (uint32_t i = 0; i < c->n_cigar; ++i) {
    uint32_t op = bam_get_cigar(b)[i];
    fprintf(f, "%u%c", bam_cigar_oplen(op), bam_cigar_opchr(op));
  }
  fputc('\t', f);
  if (c->mtid < 0) fputc('*', f);
  else if (c->mtid == c->tid) fputc('=', f);
  else fputs(h->target_name[c->mtid], f);
  fprintf(f, "\t%" PRId64 "\t%" PRId64 "\t", c->mpos + 1, c->isize);
  if (c->l_qseq <= 0) {
    fputs("*\t*", f);
  } else {
    const uint8_t *seq = bam_get_seq(b), *q = bam_get_qual(b);
    for (int32_t i = 0; i < c->l_qseq; ++i) fputc("=ACMGRSVTWYHKDBN"[bam_seqi(seq, i)], f);
    fputc('\t', f);
    if (q[0] == 0xff) fputc('*', f); /* BAM 4.2.3: qualities absent */
    else
      for (int32_t i = 0; i < c->l_qseq; ++i) fputc(q[i] + 33, f);
  }
  const uint8_t *p = bam_get_aux(b), *end = b->data + b->l_data;
  while (p + 3 <= end) {
    int sz = aux_value_size(p + 2, end);
    if (sz < 0) return -1;
    const uint8_t *v = p + 3;
    fprintf(f, "\t%c%c:", p[0], p[1]);
    switch (p[2]) {
      case 'A': fprintf(f, "A:%c", v[0]); break;
      case 'c': fprintf(f, "i:%d", (int8_t)v[0]); break;
      case 'C': fprintf(f, "i:%u", v[0]); break;
      case 's': fprintf(f, "i:%d", (int16_t)(v[0] | v[1] << 8)); break;
      case 'S': fprintf(f, "i:%u", (unsigned)(v[0] | v[1] << 8)); break;
      case 'i': fprintf(f, "i:%d", (int32_t)((uint32_t)v[0] | (uint32_t)v[1] << 8 | (uint32_t)v[2] << 16 | (uint32_t)v[3] << 24)); break;
      case 'I': fprintf(f, "i:%u", (uint32_t)v[0] | (uint32_t)v[1] << 8 | (uint32_t)v[2] << 16 | (uint32_t)v[3] << 24); break;
      case 'f': { float x; memcpy(&x, v, 4); fprintf(f, "f:%g", x); break; }
      default: fprintf(f, "%c:%s", p[2], (const char *)v); break; /* Z, H */
    }
    p += 3 + sz;
  }
  fputc('\n', f);
  return ferror(f) ? -1 : 0;
}
