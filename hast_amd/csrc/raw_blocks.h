// raw_blocks.h -- one input file's raw bytes on their way into a carried-block feed (hast_rs of classify_read, hast_sq_feed of
// unshared_kmers; carry_feed.h is the machine under both).  Host only.
#pragma once
#include <fcntl.h>
#include <unistd.h>

#include "../../include/hast.h"
#include "ingest.h"

namespace hast {

// The three ways a file's bytes reach a feed's block.  gz_on_device: inflated on the GPU straight into the device block (hast_gz_*);
// gz_on_host: inflated by BlockSource and copied into the pinned block; plain: read into the pinned block.  A BlockSource block is one
// feed block (never re-packed across BlockSource blocks), a plain file comes in full blocks until the short one, and only a read that
// gives nothing ends the stream (include/hast.h).
class RawBlocks {
  public:
    enum Kind { closed, gz_on_device, gz_on_host, plain };
    ~RawBlocks() { close(); }
    // gz: the name says gzip (the caller's rule); on the device if gz_ctx is there and hast_gz_open takes the file (BGZF, not gzip,
    // unreadable: the host decoders' words then).  false: *err says what could not be opened
    bool open(const std::string &path, bool gz, hast_ctx *gz_ctx, size_t block, std::string *err) {
        close();
        block_ = block;
        if (gz && gz_ctx && hast_gz_open(gz_ctx, path.c_str(), &z_) == HAST_OK) kind_ = gz_on_device;
        else if (gz && src_.open(path, block)) kind_ = gz_on_host;
        else if (!gz && (fd_ = ::open(path.c_str(), O_RDONLY)) >= 0) kind_ = plain;
        else *err = "cannot open " + path;
        return kind_ != closed;
    }
    Kind kind() const { return kind_; }
    // the next up to block bytes into the pinned block h; false: *err says why the input cannot be read on
    bool read_host(uint8_t *h, size_t *got, std::string *err) {
        *got = 0;
        while (kind_ == plain && *got < block_) {
            const ssize_t k = ::read(fd_, h + *got, block_ - *got);
            if (k < 0 && errno == EINTR) continue;
            if (k < 0) *err = strerror(errno);
            if (k <= 0) return k == 0;
            *got += (size_t)k;
        }
        if (kind_ == plain) return true;
        std::vector<char> blk = src_.next();         // (opened with the feed's block: a block of the source's is one of the feed's)
        if (blk.empty()) return (*err = src_.error()).empty();
        *got = blk.size() - BlockSource::kFrontPad;
        memcpy(h, blk.data() + BlockSource::kFrontPad, *got);
        src_.recycle(std::move(blk));
        return true;
    }
    // ... into the device block d, by kernels on fill_stream; false: hast_last_error()
    bool read_device(uint8_t *d, hast_stream fill_stream, size_t *got) { return hast_gz_read_device(z_, d, block_, got, fill_stream) == HAST_OK; }
    void close() {                                 // (gz_on_device: once every block is framed -- the decoder's kernels wrote them)
        if (kind_ == gz_on_device) hast_gz_close(z_);
        if (kind_ == gz_on_host) src_.close();
        if (kind_ == plain) ::close(fd_);
        kind_ = closed;
    }

  private:
    Kind kind_ = closed;
    size_t block_ = 0;
    hast_gz *z_ = nullptr;
    int fd_ = -1;
    BlockSource src_;
};

}  // namespace hast
