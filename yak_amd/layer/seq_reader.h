/* seq_reader.h -- the records of a FASTA or FASTQ file for the layers above libyak_amd.so, host only and HIP-free: a short
 * reader of kseq's grammar through gzread (plain, gzip, `-` or no name for stdin), because the engine's reader (../csrc/yak_host.h) cannot be
 * included from a layer above it.  A header starts with '>' or '@'; its name runs to the first white space and its comment from behind that one
 * character to the end of the line.  The sequence is every line up to one that starts with '>', '@' or '+'; behind '+' the quality runs until it
 * covers the sequence's length, and a quality of another length ends the file in front of its record, as it does in kseq.  Empty lines are skipped;
 * line ends may be "\n" or "\r\n".  A reader that keeps the quality gives its text (`yak-amd correct` writes the records out again); one that does
 * not leaves `qual` empty and only counts its length (`yak-amd paths`).  path.hip, correct.hip and the two model programs
 * (tests/tools/path_model_check.cpp, tools/correct_model_check.cpp) share it. */
#ifndef YAKAMD_SEQ_READER_H
#define YAKAMD_SEQ_READER_H
#include <string.h>
#include <zlib.h>
#include <string>

struct seq_record_t { std::string name, comment, seq, qual; };

class SeqReader {
public:
	explicit SeqReader(bool keep_qual) : fp_(0), at_(0), end_(0), keep_qual_(keep_qual), eof_(false), pending_(false), bad_(false) {}
	~SeqReader() { close(); }
	bool open(const char *fn)
	{
		close();
		fp_ = fn && strcmp(fn, "-") != 0 ? gzopen(fn, "rb") : gzdopen(0, "rb");
		if (fp_) gzbuffer(fp_, 1u << 18);
		at_ = end_ = 0; eof_ = pending_ = bad_ = false;
		return fp_ != 0;
	}
	void close() { if (fp_) gzclose(fp_); fp_ = 0; }
	bool failed() const { return bad_; }                          /* the inflater reported an error */
	bool keeps_qual() const { return keep_qual_; }
	/* the next record; false at the end */
	bool next(seq_record_t &r)
	{
		if (!pending_) {
			while (line()) if (!line_.empty() && (line_[0] == '>' || line_[0] == '@')) { pending_ = true; break; }
			if (!pending_) return false;
		}
		pending_ = false;
		size_t e = 1;
		while (e < line_.size() && !is_space(line_[e])) ++e;
		r.name.assign(line_, 1, e - 1);
		r.comment.assign(line_, e < line_.size() ? e + 1 : e, std::string::npos);
		r.seq.clear(); r.qual.clear();
		while (line()) {
			if (line_.empty()) continue;
			const char c = line_[0];
			if (c == '>' || c == '@') { pending_ = true; return true; }
			if (c == '+') {
				size_t q = 0;
				while (q < r.seq.size() && line()) { q += line_.size(); if (keep_qual_) r.qual += line_; }
				if (q != r.seq.size()) { eof_ = true; at_ = end_ = 0; return false; }      /* as kseq: a quality of another length ends the file */
				return true;
			}
			r.seq += line_;
		}
		return true;
	}

private:
	static bool is_space(char c) { return c == ' ' || c == '\t' || c == '\v' || c == '\f' || c == '\r' || c == '\n'; }
	bool fill()
	{
		if (eof_) return false;
		const int n = gzread(fp_, buf_, (unsigned)sizeof buf_);
		if (n < 0) bad_ = true;
		if (n <= 0) { eof_ = true; return false; }
		at_ = 0; end_ = (size_t)n;
		return true;
	}
	/* the next line into line_, without its end; false when nothing is left */
	bool line()
	{
		line_.clear();
		bool any = false;
		for (;;) {
			if (at_ == end_ && !fill()) break;
			any = true;
			const char *nl = (const char*)memchr(buf_ + at_, '\n', end_ - at_);
			if (nl) { line_.append(buf_ + at_, (size_t)(nl - (buf_ + at_))); at_ = (size_t)(nl - buf_) + 1; break; }
			line_.append(buf_ + at_, end_ - at_);
			at_ = end_;
		}
		if (!line_.empty() && line_[line_.size() - 1] == '\r') line_.erase(line_.size() - 1);
		return any;
	}
	gzFile fp_;
	char buf_[1 << 16];
	size_t at_, end_;
	const bool keep_qual_;
	bool eof_, pending_, bad_;
	std::string line_;
};
#endif
