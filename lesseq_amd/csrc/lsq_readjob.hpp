// What the loader hands a read format's device parser (lsq_mrf_device.hpp, lsq_sam_device.hpp, lsq_bam_device.hpp); not a public header.
// Needs: lsq_device.hpp (lsq_ctx, DevBuf).  Gives: the parameter structs of the parsers' kernels -- the staged text (MrfText), the
// dictionaries (MrfDict), the lists of work a tile kernel hands on (MrfHandOff), the parsed arrays of lsq_mrf_parse_device (MrfOut), a
// BAM file's inflated stream (BamView) -- and the job a format's front end is launched with (TextJob).
#pragma once
#include "lsq_device.hpp"

struct MrfText {
	const unsigned char *text;
	unsigned long long len;
	const unsigned long long *tile_base;
	unsigned has_header;
	unsigned long long first_line;            // the number of data line 0 in the whole file (read name "read-<L>")
	unsigned long long n_lines;
};

struct MrfDict {
	const unsigned *chrom_hash;             // open addressing, 0 = empty; 32-bit FNV-1a of the name
	const unsigned *chrom_id;
	const unsigned *name_off;               // per chromosome id, into names
	const char *names;
	unsigned mask, n_chrom, names_bytes;
	unsigned long long *strand_tab;         // 256 slots
};

// A line that began more than MRF_LB bytes ahead of its tile: its data line index, first byte and length.  At most one per tile.
struct MrfLongLine { unsigned long long i, start, n; };

// lists of work the fast kernel hands on: counts[0] tiles, counts[1] lines, counts[2] set when the line list ran over
struct MrfHandOff {
	unsigned *counts;
	unsigned *tiles; unsigned tile_cap;
	MrfLongLine *lines; unsigned line_cap;
};

struct MrfOut {
	unsigned long long *blk_off;
	unsigned *line_no;
	int *blk_start, *blk_end;
	unsigned short *blk_chrom;
	unsigned char *blk_strand;
};

// what the record kernels of a BAM file see: the inflated stream, the records' offsets, the reference table
struct BamView {
	const unsigned char *s;
	unsigned long long len;
	const unsigned long long *rec_off;
	const unsigned *ref_cid;                 // per refID: chromosome id, MRF_NOCHROM, or "its records make no read"
	long long n_ref;
};

// What an opened read file (lsq_readfile.hip: ReadSource) hands its format's launches: the text or the records, the dictionaries and
// the error words, the hand-off lists.
struct TextJob {
	lsq_ctx *c;
	MrfText X;                              // (a BAM file: no text; n_lines records, first_line the number of record 0)
	BamView R;
	MrfDict D;
	unsigned long long *err;
	MrfHandOff H;
	unsigned n_tiles;
	bool all_slow;                          // every tile through the format's byte-walking kernel: the front end's choice, or the line list ran over
	unsigned counts[4];                     // H.counts as the routing pass left them (the front end's record reads them)
	DevBuf<unsigned long long> tab64;       // tables of the format's own, made by its prepare (MRF: the fast kernel's dictionary)
	DevBuf<unsigned short> tab16;
};
