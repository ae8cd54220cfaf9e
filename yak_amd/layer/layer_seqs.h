/* layer_seqs.h -- the sequence front end that `yak-amd paths` and `yak-amd correct` share, beside layer_host.h and not in it
 * because it needs zlib, which walk, gfa, bubble and clean do not link: a chunk of whole sequences as a host image, the three device buffers it is
 * uploaded to, and the loop that reads a file's records (seq_reader.h) into chunks of chunk_size bases and hands each to the command.  The image
 * holds every sequence followed by '\n', off[] and len[] say where; the names stay beside them for the command's texts, and the comments and
 * qualities too where the reader keeps the quality: a command that writes the records out again needs both, one that does not needs neither. */
#ifndef YAKAMD_LAYER_SEQS_H
#define YAKAMD_LAYER_SEQS_H
#include "layer_host.h"
#include "seq_reader.h"

namespace {

inline u64 up16(u64 n) { return (n + 15) & ~(u64)15; }

struct SeqChunk {
	const bool whole;                                              /* comment[] and qual[] are kept, not name[] alone */
	std::vector<std::string> name, comment, qual;
	std::vector<char> img;
	std::vector<uint64_t> off;
	std::vector<uint32_t> len;
	uint64_t bases = 0;
	explicit SeqChunk(bool whole_) : whole(whole_) {}
	void clear() { name.clear(); comment.clear(); qual.clear(); img.clear(); off.clear(); len.clear(); bases = 0; }
	/* r's sequence goes behind the image and stays in r, whose buffer the reader fills again; what is kept of the rest moves out of r */
	void add(seq_record_t &r)
	{
		off.push_back(img.size());
		len.push_back((uint32_t)r.seq.size());
		img.insert(img.end(), r.seq.begin(), r.seq.end());
		img.push_back('\n');
		bases += r.seq.size();
		name.push_back(std::move(r.name));
		if (whole) { comment.push_back(std::move(r.comment)); qual.push_back(std::move(r.qual)); }
	}
};

struct SeqChunkDev {
	DevBuf img, off, len;
	/* the chunk's image, padded with '\n' to a multiple of 16 bytes, its offsets and its lengths into device memory; *n_bytes = the image's bytes
	 * without the padding; *copy_ms, where the command keeps such a clock, grows by the time of the three copies alone */
	int upload(const char *who, SeqChunk &c, size_t *n_bytes, double *copy_ms)
	{
		const size_t n = c.img.size(), n_seq = c.name.size();
		c.img.resize((size_t)up16(n), '\n');
		if (!img.need(c.img.size()) || !off.need(n_seq * 8) || !len.need(n_seq * 4)) return fail("%s: no device memory for a chunk of %zu bytes", who, n);
		const double t0 = now_ms();
		HIPCK(hipMemcpy(img.p, c.img.data(), c.img.size(), hipMemcpyHostToDevice));
		HIPCK(hipMemcpy(off.p, c.off.data(), n_seq * 8, hipMemcpyHostToDevice));
		HIPCK(hipMemcpy(len.p, c.len.data(), n_seq * 4, hipMemcpyHostToDevice));
		if (copy_ms) *copy_ms += now_ms() - t0;
		*n_bytes = n;
		return 0;
	}
};

/* The records of rd, which has fn open, in chunks of whole sequences: run(chunk, last) is called when chunk_size bases are in, with last = false,
 * and once more at the end of the file with what is left, which may be nothing, and last = true; the chunk is emptied behind every call.  *read_ms,
 * where the command keeps such a clock, grows by the time of the reader and the image.  -1 after the message, in the command's name `who`, for a
 * sequence whose length is no 32-bit number, for what run refuses (it has said why), for an input the inflater gave up on and for host memory
 * that ran out */
template<class Run>
int seq_chunks(const char *who, SeqReader &rd, const char *fn, int64_t chunk_size, double *read_ms, Run run)
{
	try {
		SeqChunk c(rd.keeps_qual());
		seq_record_t r;
		for (bool more = true; more;) {
			const double t0 = read_ms ? now_ms() : 0;
			more = rd.next(r);
			if (more) {
				if (r.seq.size() >= 0xffffffffull) return fail("%s: sequence '%s' has %zu bases: a length is a 32-bit number", who, r.name.c_str(), r.seq.size());
				c.add(r);
			}
			if (read_ms) *read_ms += now_ms() - t0;
			if (!more || c.bases >= (uint64_t)chunk_size) {
				if (run(c, !more) != 0) return -1;
				c.clear();
			}
		}
		if (rd.failed()) return fail("%s: '%s' is damaged: the inflater gave up", who, fn);
	} catch (const std::bad_alloc&) { return fail("%s: no host memory for a chunk", who); }
	return 0;
}

}   // namespace

#endif
