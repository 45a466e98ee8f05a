/* htslib/sam.h — STAND-IN, TEST INFRASTRUCTURE ONLY.  Our own declarations of the part of htslib's public SAM interface
 * that the reference (haowenz/FEM v0.2) uses, so that its sources compile from where they lie without htslib, which the
 * reference does not vendor (extern/htslib is an empty submodule).  htslib does no mapping arithmetic: the reference
 * fills one record per mapping (src/align.c:546-632), writes an @SQ header (src/output_queue.c:93-116) and hands both to
 * the writer.  Layouts and constants are those of the SAM/BAM specification (SAMv1, sections 1.4 and 4.2); the text
 * writer behind these declarations is oracle/ref_standin.c.  Built only by `make -C oracle ref`; never by the product.
 */
#ifndef FEM_REF_STANDIN_SAM_H_
#define FEM_REF_STANDIN_SAM_H_

#include <inttypes.h> /* the reference prints with PRIu64 and relies on this header for it */
#include <stdint.h>
#include <stdio.h>

#include "kstring.h" /* the reference's own (src/kstring.h): src/align.c uses ks_str / ks_len through this header */

/* CIGAR operations, BAM encoding: op_len << 4 | op, op an index into "MIDNSHP=X" */
#define BAM_CMATCH 0
#define BAM_CINS 1
#define BAM_CDEL 2
#define BAM_CREF_SKIP 3
#define BAM_CSOFT_CLIP 4
#define BAM_CHARD_CLIP 5
#define BAM_CPAD 6
#define BAM_CEQUAL 7
#define BAM_CDIFF 8
#define BAM_CIGAR_STR "MIDNSHP=X"
#define BAM_CIGAR_SHIFT 4
#define BAM_CIGAR_MASK 0xf
#define bam_cigar_op(c) ((c) & BAM_CIGAR_MASK)
#define bam_cigar_oplen(c) ((c) >> BAM_CIGAR_SHIFT)
#define bam_cigar_opchr(c) (BAM_CIGAR_STR[bam_cigar_op(c)])
#define bam_cigar_gen(l, o) ((l) << BAM_CIGAR_SHIFT | (o))

/* FLAG bits (SAMv1 1.4) */
#define BAM_FPAIRED 1
#define BAM_FPROPER_PAIR 2
#define BAM_FUNMAP 4
#define BAM_FMUNMAP 8
#define BAM_FREVERSE 16
#define BAM_FMREVERSE 32
#define BAM_FREAD1 64
#define BAM_FREAD2 128
#define BAM_FSECONDARY 256
#define BAM_FQCFAIL 512
#define BAM_FDUP 1024
#define BAM_FSUPPLEMENTARY 2048

typedef struct {
  int64_t pos;  /* 0-based leftmost coordinate */
  int32_t tid;  /* index of the reference sequence in the header */
  uint16_t bin;
  uint8_t qual; /* MAPQ */
  uint8_t l_extranul;
  uint16_t flag;
  uint16_t l_qname; /* name + its NULs */
  uint32_t n_cigar;
  int32_t l_qseq;
  int32_t mtid;
  int64_t mpos;
  int64_t isize;
} bam1_core_t;

/* data: qname (l_qname bytes) | cigar (4 n_cigar) | seq ((l_qseq + 1) / 2 nibble pairs) | qual (l_qseq) | aux */
typedef struct {
  bam1_core_t core;
  uint64_t id;
  uint8_t *data;
  int l_data;
  uint32_t m_data;
  uint32_t mempolicy;
} bam1_t;

typedef struct {
  int32_t n_targets;
  int32_t ignore_sam_err;
  size_t l_text;
  uint32_t *target_len;
  const int8_t *cigar_tab;
  char **target_name;
  char *text;
  void *sdict;
  void *hrecs;
  uint32_t ref_count;
} sam_hdr_t;

typedef struct {
  FILE *fp;
} samFile;

#define bam_get_qname(b) ((char *)(b)->data)
#define bam_get_cigar(b) ((uint32_t *)((b)->data + (b)->core.l_qname))
#define bam_get_seq(b) ((b)->data + ((b)->core.n_cigar << 2) + (b)->core.l_qname)
#define bam_get_qual(b) ((b)->data + ((b)->core.n_cigar << 2) + (b)->core.l_qname + (((b)->core.l_qseq + 1) >> 1))
#define bam_get_aux(b) \
  ((b)->data + ((b)->core.n_cigar << 2) + (b)->core.l_qname + (((b)->core.l_qseq + 1) >> 1) + (b)->core.l_qseq)
#define bam_get_l_aux(b) \
  ((b)->l_data - ((b)->core.n_cigar << 2) - (b)->core.l_qname - (b)->core.l_qseq - (((b)->core.l_qseq + 1) >> 1))
/* base i of a nibble-packed sequence: the earlier base in the high nibble */
#define bam_seqi(s, i) ((s)[(i) >> 1] >> ((~(i) & 1) << 2) & 0xf)
#define bam_set_seqi(s, i, b) \
  ((s)[(i) >> 1] = (uint8_t)(((s)[(i) >> 1] & (0xf0 >> ((~(i) & 1) << 2))) | ((b) << ((~(i) & 1) << 2))))

/* character -> nibble code of "=ACMGRSVTWYHKDBN", either case; everything else is N (15) */
extern const unsigned char seq_nt16_table[256];

bam1_t *bam_init1(void);
void bam_destroy1(bam1_t *b);
int bam_aux_update_int(bam1_t *b, const char tag[2], int64_t val);
int bam_aux_update_str(bam1_t *b, const char tag[2], int len, const char *data);

samFile *sam_open_format(const char *path, const char *mode, const void *format);
int sam_close(samFile *fp);
sam_hdr_t *sam_hdr_init(void);
void sam_hdr_destroy(sam_hdr_t *h);
int sam_hdr_write(samFile *fp, const sam_hdr_t *h);
int sam_write1(samFile *fp, const sam_hdr_t *h, const bam1_t *b);

#endif /* FEM_REF_STANDIN_SAM_H_ */
