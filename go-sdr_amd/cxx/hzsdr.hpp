// hzsdr.hpp -- C++ host-side mirror of the reference's Go interfaces for the hot
// path, over the C ABI of include/hzsdr.h (the reference is compiled code and the
// image has no Go toolchain, so the compiled-language host layer is C++; the cgo
// package in INTEGRATION.md is this file transliterated).
//
// Names follow the reference: sdr::Reader (reader.go:39-51), sdr::ReadFull
// (reader.go:72), stream::ReadTransformer (stream/read_transformer.go:45-137),
// stream::ConvertReader / DecimateReader / DownsampleReader / ShiftReader / Gain /
// Multiply / Add / ConvolutionReader / ReadBeamform (stream/*.go), sdr::LookupTable
// (iq_lookup_table.go), fft::Planner / Plan / TransformOnce / Convolve / CrossCorrelate /
// ConvolveFreq (fft/*.go), plus stream::Chain, the fused form the north star adds.
// Errors are the reference's sentinels, thrown as hzsdr::Error
// carrying the status code.  Buffers are host memory (a HZSDR_MEM_HOST context),
// as Go slices would be.
#pragma once
#include <complex>
#include <cstdint>
#include <cstring>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "../../include/hzsdr.h"
#include "../../include/hzsdr_channelizer.h"
#include "../../include/hzsdr_resampler.h"
#include "../../include/hzsdr_demod.h"
#include "../../include/hzsdr_tuner.h"
#include "../../include/hzsdr_chanbank.h"
#include "../../include/hzsdr_covar.h"
#include "../../include/hzsdr_iir.h"
#include "../../include/hzsdr_symsync.h"
#include "../../include/hzsdr_carrier.h"
#include "../../include/hzsdr_agc.h"
#include "../../include/hzsdr_equalizer.h"
#include "../../include/hzsdr_framesync.h"
#include "../../include/hzsdr_hdlc.h"
#include "../../include/hzsdr_viterbi.h"
#include "../../include/hzsdr_ldpc.h"
#include "../../include/hzsdr_demap.h"
#include "../../include/hzsdr_rs.h"
#include "../../include/hzsdr_softframe.h"
#include "../../include/hzsdr_spectrum.h"
#include "../../include/hzsdr_synthesizer.h"

namespace hzsdr {

struct Error : std::runtime_error {
    int status;
    Error(int s, const std::string &m) : std::runtime_error(m), status(s) {}
};
struct Eof : std::exception {};

inline void check(hzsdr_ctx *ctx, int rc) {
    if (rc == HZSDR_OK) return;
    std::string m = hzsdr_strerror(rc);
    if (ctx && *hzsdr_last_error(ctx)) m += std::string(": ") + hzsdr_last_error(ctx);
    throw Error(rc, m);
}

// sdr.Samples: a typed view over caller-owned memory (iq.go:59-87)
struct Samples {
    int format = 0;
    void *data = nullptr;
    size_t length = 0;  // IQ samples
    size_t size() const { return length * (size_t)hzsdr_format_size(format); }
    Samples slice(size_t lo, size_t hi) const {
        return Samples{format, (char *)data + lo * (size_t)hzsdr_format_size(format), hi - lo};
    }
};

// sdr.MakeSamples (iq.go:128-141): owning storage + its view
struct Buffer {
    std::vector<unsigned char> bytes;
    Samples view;
    Buffer(int format, size_t n) {
        if (hzsdr_format_size(format) == 0) throw Error(HZSDR_ERR_FORMAT_UNKNOWN, hzsdr_strerror(HZSDR_ERR_FORMAT_UNKNOWN));
        bytes.assign(n * (size_t)hzsdr_format_size(format), 0);
        view = Samples{format, bytes.data(), n};
    }
};

class Context {
public:
    explicit Context(int device = 0) { check(nullptr, hzsdr_open(device, HZSDR_MEM_HOST, &c_)); }
    ~Context() { if (c_) hzsdr_close(c_); }
    Context(const Context &) = delete;
    hzsdr_ctx *raw() const { return c_; }
    // hzsdr_call_count: library calls made on this context so far
    unsigned long long CallCount() const {
        unsigned long long n = 0;
        check(c_, hzsdr_call_count(c_, &n));
        return n;
    }

    // sdr.ConvertBuffer (conv.go:55)
    size_t ConvertBuffer(Samples dst, Samples src) const {
        size_t n = 0;
        check(c_, hzsdr_convert(c_, dst.format, dst.data, dst.length, src.format, src.data, src.length, &n));
        return n;
    }
    // SamplesC64.Scale / Multiply / Add (iq_c64.go:122-136)
    void Scale(Samples s, float r) const { need_c64(s); check(c_, hzsdr_scale(c_, s.data, s.length, r)); }
    void Multiply(Samples s, float re, float im) const { need_c64(s); check(c_, hzsdr_rotate(c_, s.data, s.length, re, im)); }
    void Add(Samples a, Samples b) const { check(c_, hzsdr_add(c_, a.data, a.length, b.data, b.length, a.data, a.length)); }
    // stream.DecimateBuffer / DownsampleBuffer
    size_t DecimateBuffer(Samples to, Samples from, unsigned factor, int64_t offset) const {
        size_t n = 0;
        check(c_, hzsdr_decimate(c_, to.format, to.data, to.length, from.format, from.data, from.length, factor, offset, &n));
        return n;
    }
    size_t DownsampleBuffer(Samples to, Samples from, unsigned factor, int64_t offset) const {
        size_t n = 0;
        check(c_, hzsdr_downsample(c_, to.format, to.data, to.length, from.format, from.data, from.length, factor, offset, &n));
        return n;
    }

private:
    static void need_c64(const Samples &s) {
        if (s.format != HZSDR_FMT_C64) throw Error(HZSDR_ERR_FORMAT_UNKNOWN, hzsdr_strerror(HZSDR_ERR_FORMAT_UNKNOWN));
    }
    hzsdr_ctx *c_ = nullptr;
};

// sdr.Reader (reader.go:39-51)
struct Reader {
    virtual ~Reader() = default;
    virtual size_t Read(Samples s) = 0;
    virtual int SampleFormat() const = 0;
    virtual unsigned SampleRate() const = 0;
};
using ReaderPtr = std::shared_ptr<Reader>;

// sdr.Writer (writer.go)
struct Writer {
    virtual ~Writer() = default;
    virtual size_t Write(Samples s) = 0;
    virtual int SampleFormat() const = 0;
    virtual unsigned SampleRate() const = 0;
};
using WriterPtr = std::shared_ptr<Writer>;

// sdr.ReadFull (reader.go:72-117).  Throws Eof with nothing read, Error(short) after a partial read.
inline size_t ReadFull(Reader &r, Samples buf, size_t *partial = nullptr) {
    size_t n = 0;
    while (n < buf.length) {
        try {
            n += r.Read(buf.slice(n, buf.length));
        } catch (const Eof &) {
            if (partial) *partial = n;
            if (n > 0) throw Error(-1, "sdr: unexpected EOF");
            throw;
        }
    }
    return n;
}

// an in-memory source: mock.Sdr's Rx / a written sdr.Pipe in the reference's tests
class BufferReader : public Reader {
public:
    BufferReader(Samples data, unsigned rate, size_t max_read = 0) : d_(data), rate_(rate), max_(max_read) {}
    size_t Read(Samples s) override {
        if (s.format != d_.format) throw Error(HZSDR_ERR_FORMAT_MISMATCH, hzsdr_strerror(HZSDR_ERR_FORMAT_MISMATCH));
        size_t left = d_.length - pos_;
        if (left == 0) throw Eof();
        size_t n = left < s.length ? left : s.length;
        if (max_ && n > max_) n = max_;
        std::memcpy(s.data, d_.slice(pos_, pos_ + n).data, n * (size_t)hzsdr_format_size(d_.format));
        pos_ += n;
        return n;
    }
    int SampleFormat() const override { return d_.format; }
    unsigned SampleRate() const override { return rate_; }

private:
    Samples d_;
    unsigned rate_;
    size_t max_, pos_ = 0;
};

// stream.ReadTransformer (stream/read_transformer.go:45-137), pull-driven
class ReadTransformer : public Reader {
public:
    using Proc = std::function<size_t(Samples in, Samples out)>;
    ReadTransformer(ReaderPtr in, size_t in_len, size_t out_len, int out_fmt, unsigned out_rate, Proc p)
        : in_(std::move(in)), ibuf_(in_->SampleFormat(), in_len), obuf_(out_fmt, out_len), fmt_(out_fmt),
          rate_(out_rate), proc_(std::move(p)) {}
    size_t Read(Samples s) override {
        if (s.format != fmt_) throw Error(HZSDR_ERR_FORMAT_MISMATCH, hzsdr_strerror(HZSDR_ERR_FORMAT_MISMATCH));
        if (avail_ == 0) {
            if (done_) throw Eof();
            try {
                size_t inn = ReadFull(*in_, ibuf_.view);
                avail_ = proc_(ibuf_.view.slice(0, inn), obuf_.view);
                off_ = 0;
            } catch (const Eof &) { done_ = true; throw; }
            catch (const Error &e) { done_ = true; if (e.status == -1) throw Eof(); throw; }
        }
        size_t n = avail_ < s.length ? avail_ : s.length;
        std::memcpy(s.data, obuf_.view.slice(off_, off_ + n).data, n * (size_t)hzsdr_format_size(fmt_));
        off_ += n;
        avail_ -= n;
        return n;
    }
    int SampleFormat() const override { return fmt_; }
    unsigned SampleRate() const override { return rate_; }

private:
    ReaderPtr in_;
    Buffer ibuf_, obuf_;
    int fmt_;
    unsigned rate_;
    Proc proc_;
    size_t avail_ = 0, off_ = 0;
    bool done_ = false;
};

namespace stream {

constexpr size_t kBlock = 32 * 1024;  // stream/convert.go:43-44

// stream.ConvertReader (stream/convert.go:37-51)
inline ReaderPtr ConvertReader(const Context &x, ReaderPtr in, int to) {
    unsigned rate = in->SampleRate();
    return std::make_shared<ReadTransformer>(std::move(in), kBlock, kBlock, to, rate,
                                             [&x](Samples i, Samples o) { return x.ConvertBuffer(o, i); });
}

// stream.ConvertWriter (stream/convert.go:58-118): a Writer of `input_format` in front of `out`; every Write is
// converted in chunks of 32 Ki samples into a buffer of out's format and handed on whole.  A Write of another format
// throws ErrSampleFormatMismatch before anything is converted; "Conversion mismatch" if a chunk comes back short.
class ConvWriter : public Writer {
public:
    ConvWriter(const Context &x, WriterPtr out, int input_format)
        : x_(x), out_(std::move(out)), fmt_(input_format), buf_(out_->SampleFormat(), kBlock) {}
    size_t Write(Samples in) override {
        if (in.format != fmt_) throw Error(HZSDR_ERR_FORMAT_MISMATCH, hzsdr_strerror(HZSDR_ERR_FORMAT_MISMATCH));
        size_t n = 0;
        for (size_t i = 0; i < in.length; i += kBlock) {
            const size_t ie = i + kBlock > in.length ? in.length : i + kBlock;
            const size_t leng = x_.ConvertBuffer(buf_.view, in.slice(i, ie));
            if (ie - i != leng) throw Error(-1, "ConvertWriter: Conversion mismatch");
            n += out_->Write(buf_.view.slice(0, leng));
        }
        return n;
    }
    int SampleFormat() const override { return fmt_; }
    unsigned SampleRate() const override { return out_->SampleRate(); }

private:
    const Context &x_;
    WriterPtr out_;
    int fmt_;
    Buffer buf_;
};
inline WriterPtr ConvertWriter(const Context &x, WriterPtr out, int input_format) {
    return std::make_shared<ConvWriter>(x, std::move(out), input_format);
}

// stream.DownsampleReader (stream/downsample.go:47-64)
inline ReaderPtr DownsampleReader(const Context &x, ReaderPtr in, unsigned factor) {
    unsigned rate = in->SampleRate() / factor;
    auto offset = std::make_shared<int64_t>(0);
    return std::make_shared<ReadTransformer>(std::move(in), kBlock, kBlock, HZSDR_FMT_C64, rate,
                                             [&x, factor, offset](Samples i, Samples o) {
                                                 size_t n = x.DownsampleBuffer(o, i, factor, *offset);
                                                 *offset += (int64_t)i.length;
                                                 return n;
                                             });
}

// stream.DecimateReader (stream/decimate.go:34-55)
inline ReaderPtr DecimateReader(const Context &x, ReaderPtr in, unsigned factor) {
    unsigned rate = in->SampleRate() / factor;
    int fmt = in->SampleFormat();
    auto offset = std::make_shared<int64_t>(0);
    return std::make_shared<ReadTransformer>(std::move(in), kBlock, kBlock, fmt, rate,
                                             [&x, factor, offset](Samples i, Samples o) {
                                                 size_t n = x.DecimateBuffer(o, i, factor, *offset);
                                                 *offset += (int64_t)i.length;
                                                 return n;
                                             });
}

// stream.ShiftReader (stream/shifter.go:89-102): the closure's ts lives in an hzsdr_nco
class ShiftReaderImpl : public Reader {
public:
    ShiftReaderImpl(const Context &x, ReaderPtr r, double shift_hz) : x_(x), r_(std::move(r)), shift_(shift_hz) {
        if (r_->SampleFormat() != HZSDR_FMT_C64) throw Error(HZSDR_ERR_FORMAT_UNKNOWN, hzsdr_strerror(HZSDR_ERR_FORMAT_UNKNOWN));
        check(x_.raw(), hzsdr_nco_create(x_.raw(), r_->SampleRate(), &nco_));
    }
    ~ShiftReaderImpl() override { if (nco_) hzsdr_nco_free(nco_); }
    size_t Read(Samples s) override {
        if (s.format != HZSDR_FMT_C64) throw Error(HZSDR_ERR_FORMAT_UNKNOWN, hzsdr_strerror(HZSDR_ERR_FORMAT_UNKNOWN));
        size_t n = r_->Read(s);
        check(x_.raw(), hzsdr_nco_shift(nco_, shift_, s.data, n));
        return n;
    }
    int SampleFormat() const override { return r_->SampleFormat(); }
    unsigned SampleRate() const override { return r_->SampleRate(); }
    // hzsdr_nco_set_ulp1 (go/hip/stream.go Shifter.SetULP1): the factor within one float32 ulp of the reference's
    // instead of bit-identical to it; off by default
    void SetULP1(bool on) { check(x_.raw(), hzsdr_nco_set_ulp1(nco_, on ? 1 : 0)); }

private:
    const Context &x_;
    ReaderPtr r_;
    double shift_;
    hzsdr_nco *nco_ = nullptr;
};
inline std::shared_ptr<ShiftReaderImpl> ShiftReader(const Context &x, ReaderPtr r, double shift_hz) {
    return std::make_shared<ShiftReaderImpl>(x, std::move(r), shift_hz);
}

// stream.Gain (stream/gain.go:30-57)
class GainReader : public Reader {
public:
    GainReader(const Context &x, ReaderPtr r, float v) : x_(x), r_(std::move(r)), v_(v) {}
    size_t Read(Samples s) override {
        size_t n = r_->Read(s);
        x_.Scale(s.slice(0, n), v_);
        return n;
    }
    int SampleFormat() const override { return r_->SampleFormat(); }
    unsigned SampleRate() const override { return r_->SampleRate(); }

private:
    const Context &x_;
    ReaderPtr r_;
    float v_;
};
inline ReaderPtr Gain(const Context &x, ReaderPtr r, float v) { return std::make_shared<GainReader>(x, std::move(r), v); }

}  // namespace stream

// sdr.LookupTable (iq_lookup_table.go:98-150)
class LookupTable {
public:
    // NewLookupTable(inputFormat, lookup): `lookup` holds 65536 samples of the output format
    LookupTable(const Context &x, int input_format, Samples lookup) : x_(x), in_(input_format), out_(lookup.format) {
        check(x_.raw(), hzsdr_lut_create(x_.raw(), input_format, lookup.format, lookup.data, lookup.length, &t_));
    }
    ~LookupTable() { if (t_) hzsdr_lut_free(t_); }
    LookupTable(const LookupTable &) = delete;
    size_t Lookup(Samples dst, Samples src) const {
        size_t n = 0;
        check(x_.raw(), hzsdr_lut_lookup(t_, dst.format, dst.data, dst.length, src.format, src.data, src.length, &n));
        return n;
    }
    int InputFormat() const { return in_; }
    int OutputFormat() const { return out_; }

private:
    const Context &x_;
    int in_, out_;
    hzsdr_lut *t_ = nullptr;
};
// LookupTableIdentityU8 / I8 (iq_lookup_table.go:69-90): same bytes, two views
inline Buffer LookupTableIdentity(int format) {
    Buffer b(format, 65536);
    hzsdr_lut_identity(b.bytes.data());
    return b;
}

namespace fft {

enum Direction { Backward = HZSDR_FFT_BACKWARD, Forward = HZSDR_FFT_FORWARD };  // fft/fft.go:30-37

// fft.Plan (fft/fft.go:50-59): aliases the two buffers for its whole life
class Plan {
public:
    Plan(const Context &x, Samples iq, Samples frequency, Direction d) : x_(x) {
        check(x_.raw(), hzsdr_fft_plan(x_.raw(), iq.data, iq.length, frequency.data, frequency.length, (int)d, &p_));
    }
    ~Plan() { Close(); }
    Plan(const Plan &) = delete;
    void Transform() { check(x_.raw(), hzsdr_fft_transform(p_)); }
    void Close() { if (p_) { hzsdr_fft_free(p_); p_ = nullptr; } }

private:
    const Context &x_;
    hzsdr_fft *p_ = nullptr;
};
using PlanPtr = std::unique_ptr<Plan>;
// fft.Planner (fft/fft.go:45-48)
using Planner = std::function<PlanPtr(Samples iq, Samples frequency, Direction)>;
inline Planner NewPlanner(const Context &x) {
    return [&x](Samples iq, Samples f, Direction d) { return PlanPtr(new Plan(x, iq, f, d)); };
}
// fft.TransformOnce (fft/fft.go:64-75)
inline void TransformOnce(const Planner &planner, Samples iq, Samples frequency, Direction d) {
    auto p = planner(iq, frequency, d);
    p->Transform();
    p->Close();
}

// the "func() error" closures of fft/convolution.go as an object
class Closure {
public:
    Closure(const Context &x, hzsdr_conv *c) : x_(x), c_(c) {}
    ~Closure() { if (c_) hzsdr_conv_free(c_); }
    Closure(const Closure &) = delete;
    void operator()() { check(x_.raw(), hzsdr_conv_exec(c_)); }

private:
    const Context &x_;
    hzsdr_conv *c_;
};
using ClosurePtr = std::unique_ptr<Closure>;

inline ClosurePtr two_input(const Context &x, Samples dst, Samples iq1, Samples iq2, int mode) {
    hzsdr_conv *c = nullptr;
    check(x.raw(), hzsdr_convolve_create(x.raw(), dst.data, dst.length, iq1.data, iq1.length, iq2.data, iq2.length, mode, &c));
    return ClosurePtr(new Closure(x, c));
}
// fft.Convolve (fft/convolution.go:97-113) / fft.CrossCorrelate (:119-138).  The
// planner argument of the reference is the context here: the plans live in the library.
inline ClosurePtr Convolve(const Context &x, Samples dst, Samples iq1, Samples iq2) {
    return two_input(x, dst, iq1, iq2, HZSDR_CONV_CONVOLVE);
}
inline ClosurePtr CrossCorrelate(const Context &x, Samples dst, Samples iq1, Samples iq2) {
    return two_input(x, dst, iq1, iq2, HZSDR_CONV_CROSS_CORRELATE);
}
// fft.ConvolveOnce (fft/convolution.go:200-211)
inline void ConvolveOnce(const Context &x, Samples dst, Samples iq1, Samples iq2) { (*Convolve(x, dst, iq1, iq2))(); }
// fft.ConvolveFreq (fft/convolution.go:150-192)
inline ClosurePtr ConvolveFreq(const Context &x, Samples dst, Samples src, Samples freq) {
    hzsdr_conv *c = nullptr;
    check(x.raw(), hzsdr_convolve_freq_create(x.raw(), dst.data, dst.length, src.data, src.length, freq.data, freq.length, &c));
    return ClosurePtr(new Closure(x, c));
}

}  // namespace fft

namespace stream {

// stream.Multiply (stream/multiply.go:27-238): c64 in place, u8 / i8 through the
// rotation table; SetMultiplier is the reference's undocumented setter (:34-36)
class MultiplyReader : public Reader {
public:
    MultiplyReader(const Context &x, ReaderPtr r, float re, float im) : x_(x), r_(std::move(r)), re_(re), im_(im) {
        const int f = r_->SampleFormat();
        if (f == HZSDR_FMT_U8 || f == HZSDR_FMT_I8) check(x_.raw(), hzsdr_rotlut_create(x_.raw(), f, re, im, &t_));
        else if (f != HZSDR_FMT_C64) throw Error(HZSDR_ERR_FORMAT_UNKNOWN, hzsdr_strerror(HZSDR_ERR_FORMAT_UNKNOWN));
    }
    ~MultiplyReader() override { if (t_) hzsdr_rotlut_free(t_); }
    void SetMultiplier(float re, float im) {
        re_ = re;
        im_ = im;
        if (t_) check(x_.raw(), hzsdr_rotlut_set_multiplier(t_, re, im));
    }
    size_t Read(Samples s) override {
        if (s.format != r_->SampleFormat()) throw Error(HZSDR_ERR_FORMAT_MISMATCH, hzsdr_strerror(HZSDR_ERR_FORMAT_MISMATCH));
        size_t n = r_->Read(s);
        if (t_) check(x_.raw(), hzsdr_rotlut_apply(t_, s.data, n));
        else if (!(re_ == 1.0f && im_ == 0.0f)) x_.Multiply(s.slice(0, n), re_, im_);  // multiply.go:59-62
        return n;
    }
    int SampleFormat() const override { return r_->SampleFormat(); }
    unsigned SampleRate() const override { return r_->SampleRate(); }

private:
    const Context &x_;
    ReaderPtr r_;
    float re_, im_;
    hzsdr_rotlut *t_ = nullptr;
};
inline std::shared_ptr<MultiplyReader> Multiply(const Context &x, ReaderPtr r, float re, float im) {
    return std::make_shared<MultiplyReader>(x, std::move(r), re, im);
}

// stream.Add (stream/add.go:41-185)
class AddReader : public Reader {
public:
    AddReader(const Context &x, std::vector<ReaderPtr> rs) : x_(x), rs_(std::move(rs)) {}
    size_t Read(Samples s) override {
        if (failed_) throw Error(failed_, hzsdr_strerror(failed_));
        if (s.format != HZSDR_FMT_C64 && s.format != HZSDR_FMT_I16 && s.format != HZSDR_FMT_I8)
            throw Error(HZSDR_ERR_FORMAT_UNKNOWN, hzsdr_strerror(HZSDR_ERR_FORMAT_UNKNOWN));
        std::vector<Buffer> bufs;
        std::vector<const void *> ptrs;
        bufs.reserve(rs_.size());
        for (auto &r : rs_) {
            bufs.emplace_back(s.format, s.length);
            try {
                ReadFull(*r, bufs.back().view);  // add.go:147: short input poisons the reader
            } catch (const Eof &) { failed_ = -1; throw; }
            catch (const Error &e) { failed_ = e.status; throw; }
            ptrs.push_back(bufs.back().view.data);
        }
        check(x_.raw(), hzsdr_sum(x_.raw(), s.format, s.data, ptrs.data(), (int)ptrs.size(), s.length));
        return s.length;
    }
    int SampleFormat() const override { return rs_[0]->SampleFormat(); }
    unsigned SampleRate() const override { return rs_[0]->SampleRate(); }

private:
    const Context &x_;
    std::vector<ReaderPtr> rs_;
    int failed_ = 0;
};
inline ReaderPtr Add(const Context &x, std::vector<ReaderPtr> rs) {
    if (rs.empty()) throw Error(HZSDR_ERR_INVALID_ARGUMENT, "stream.Add: No readers passed");
    if (rs.size() == 1) return rs[0];
    const int f = rs[0]->SampleFormat();
    if (f != HZSDR_FMT_C64 && f != HZSDR_FMT_I16 && f != HZSDR_FMT_I8)
        throw Error(HZSDR_ERR_FORMAT_UNKNOWN, hzsdr_strerror(HZSDR_ERR_FORMAT_UNKNOWN));
    for (auto &r : rs) {
        if (r->SampleFormat() != f) throw Error(HZSDR_ERR_INVALID_ARGUMENT, "stream.Add: Readers are not all the same format");
        if (r->SampleRate() != rs[0]->SampleRate()) throw Error(HZSDR_ERR_INVALID_ARGUMENT, "stream.Add: Readers are not all the same rate");
    }
    return std::make_shared<AddReader>(x, std::move(rs));
}

// stream.ConvolutionReader (stream/convolution.go:36-82): `filter` is in the frequency domain
inline ReaderPtr ConvolutionReader(const Context &x, ReaderPtr r, Samples filter) {
    if (r->SampleFormat() != HZSDR_FMT_C64) throw Error(HZSDR_ERR_FORMAT_UNKNOWN, hzsdr_strerror(HZSDR_ERR_FORMAT_UNKNOWN));
    const size_t n = filter.length;
    auto iq = std::make_shared<Buffer>(HZSDR_FMT_C64, n);
    std::shared_ptr<fft::Closure> conv = fft::ConvolveFreq(x, iq->view, iq->view, filter);
    unsigned rate = r->SampleRate();
    return std::make_shared<ReadTransformer>(std::move(r), n, n, HZSDR_FMT_C64, rate, [iq, conv](Samples in, Samples out) {
        std::memcpy(iq->view.data, in.data, in.size());
        (*conv)();
        std::memcpy(out.data, iq->view.data, in.size());
        return in.length;
    });
}

// stream.ReadBeamform / Beamform (stream/beamform.go:131-171).  One fused kernel per
// Read instead of K convert + K multiply + K+1 add passes; same arithmetic order.
class Beamform : public Reader {
public:
    Beamform(const Context &x, std::vector<ReaderPtr> rs, std::vector<std::complex<float>> angles)
        : x_(x), rs_(std::move(rs)), w_(rs_.size(), {1.0f, 0.0f}) {
        for (auto &r : rs_)
            if (r->SampleFormat() != rs_[0]->SampleFormat() || r->SampleRate() != rs_[0]->SampleRate())
                throw Error(HZSDR_ERR_INVALID_ARGUMENT, "stream.Add: Readers are not all the same format / rate");
        SetPhaseAngles(angles);
    }
    // returns false where the reference returns its length error (beamform.go:132-134)
    bool SetPhaseAngles(const std::vector<std::complex<float>> &angles) {
        if (angles.size() != rs_.size()) return false;
        w_ = angles;
        return true;
    }
    size_t Read(Samples s) override {
        if (s.format != HZSDR_FMT_C64) throw Error(HZSDR_ERR_FORMAT_MISMATCH, hzsdr_strerror(HZSDR_ERR_FORMAT_MISMATCH));
        const int f = rs_[0]->SampleFormat();
        std::vector<Buffer> bufs;
        std::vector<const void *> ptrs;
        bufs.reserve(rs_.size());
        for (auto &r : rs_) {
            bufs.emplace_back(f, s.length);
            ReadFull(*r, bufs.back().view);
            ptrs.push_back(bufs.back().view.data);
        }
        check(x_.raw(), hzsdr_beamform(x_.raw(), s.data, f, ptrs.data(), reinterpret_cast<const float *>(w_.data()),
                                       (int)ptrs.size(), s.length));
        return s.length;
    }
    int SampleFormat() const override { return HZSDR_FMT_C64; }
    unsigned SampleRate() const override { return rs_[0]->SampleRate(); }

private:
    const Context &x_;
    std::vector<ReaderPtr> rs_;
    std::vector<std::complex<float>> w_;
};
inline std::shared_ptr<Beamform> ReadBeamform(const Context &x, std::vector<ReaderPtr> rs, std::vector<std::complex<float>> angles) {
    return std::make_shared<Beamform>(x, std::move(rs), std::move(angles));
}
// stream.BeamformAngles (stream/beamform.go:104-128)
inline std::vector<std::complex<float>> BeamformAngles(double frequency_hz, double angle_deg, const std::vector<double> &distances) {
    std::vector<std::complex<float>> out(distances.size());
    hzsdr_beamform_angles(frequency_hz, angle_deg, distances.data(), (int)distances.size(), reinterpret_cast<float *>(out.data()));
    return out;
}

// The fused form of a reader chain (north_star): ops are appended in reader order,
// Run consumes one resident buffer per call; NCO time and FIR history persist.
class Chain {
public:
    Chain(const Context &x, int src_format, uint64_t sample_rate) : x_(x) { check(x_.raw(), hzsdr_chain_create(x_.raw(), src_format, sample_rate, &c_)); }
    ~Chain() { if (c_) hzsdr_chain_free(c_); }
    Chain(const Chain &) = delete;
    Chain &Shift(double hz) { check(x_.raw(), hzsdr_chain_shift(c_, hz)); return *this; }
    Chain &Gain(float r) { check(x_.raw(), hzsdr_chain_gain(c_, r)); return *this; }
    Chain &Multiply(float re, float im) { check(x_.raw(), hzsdr_chain_rotate(c_, re, im)); return *this; }
    Chain &Decimate(unsigned f) { check(x_.raw(), hzsdr_chain_decimate(c_, f)); return *this; }
    Chain &Downsample(unsigned f) { check(x_.raw(), hzsdr_chain_downsample(c_, f)); return *this; }
    Chain &Convolution(Samples filter, unsigned decimate = 1) { check(x_.raw(), hzsdr_chain_convolution(c_, filter.data, filter.length, decimate)); return *this; }
    Chain &FirDecimate(const std::vector<std::complex<float>> &taps, unsigned d) {
        check(x_.raw(), hzsdr_chain_fir_decimate(c_, reinterpret_cast<const float *>(taps.data()), taps.size(), d));
        return *this;
    }
    // hzsdr_chain_pipeline: consecutive Run calls on the matrix path overlap (the input must be complete at call time)
    Chain &Pipeline(bool on = true) { check(x_.raw(), hzsdr_chain_pipeline(c_, on ? 1 : 0)); return *this; }
    // -> (consumed, produced)
    std::pair<size_t, size_t> Run(Samples in, Samples out) {
        size_t used = 0, made = 0;
        check(x_.raw(), hzsdr_chain_run(c_, in.data, in.length, out.data, out.length, &used, &made));
        return {used, made};
    }
    void Reset() { check(x_.raw(), hzsdr_chain_reset(c_)); }
    // every sample mixed before the FIR (reference order) instead of after it
    Chain &MixInOrder(bool in_order = true) { check(x_.raw(), hzsdr_chain_mix_in_order(c_, in_order ? 1 : 0)); return *this; }
    hzsdr_chain *raw() const { return c_; }
    const Context &context() const { return x_; }

private:
    const Context &x_;
    hzsdr_chain *c_ = nullptr;
};

// The pinned ring in front of a chain: what stream.RingBuffer with an IQBufferAllocator of
// hipHostMalloc memory is to a driver callback (stream/ring.go:48-69, :337-392).
class Ring {
public:
    Ring(Chain &chain, size_t slot_length, int slots) : x_(chain.context()) {
        check(x_.raw(), hzsdr_ring_create(chain.raw(), slot_length, slots, &r_));
        void *base = nullptr;
        size_t n = 0;
        check(x_.raw(), hzsdr_ring_iq_buffer(r_, &base, &n, &slot_length_));
        base_ = base;
        total_ = n;
    }
    ~Ring() { if (r_) hzsdr_ring_free(r_); }
    Ring(const Ring &) = delete;
    // the whole IQBufferAllocator region, in the chain's source format
    Samples IQBuffer(int format) const { return Samples{format, base_, total_}; }
    // write cursor: the next slot's memory
    Samples Acquire(int format, int *slot) {
        void *p = nullptr;
        check(x_.raw(), hzsdr_ring_acquire(r_, slot, &p));
        return Samples{format, p, slot_length_};
    }
    void Submit(int slot, size_t n) { check(x_.raw(), hzsdr_ring_submit(r_, slot, n)); }
    // `count` acquired slots, first_slot the oldest, n samples each, as ONE call of the chain (hzsdr_ring_submit_many)
    void SubmitMany(int first_slot, int count, size_t n) { check(x_.raw(), hzsdr_ring_submit_many(r_, first_slot, count, n)); }
    void Release(int slot) { check(x_.raw(), hzsdr_ring_release(r_, slot)); }  // the acquired slot, unused
    // read cursor: the oldest submitted slot's output (complex64), valid until that slot is resubmitted
    Samples Pop() {
        const void *p = nullptr;
        size_t n = 0;
        check(x_.raw(), hzsdr_ring_pop(r_, &p, &n));
        return Samples{HZSDR_FMT_C64, const_cast<void *>(p), n};
    }
    int InFlight() const { return hzsdr_ring_in_flight(r_); }

private:
    const Context &x_;
    hzsdr_ring *r_ = nullptr;
    void *base_ = nullptr;
    size_t total_ = 0, slot_length_ = 0;
};


// ---- nested Readers that fuse into one chain and read ahead (go/hip/fused.go is this, in Go) ---------------------------
// The constructors of `Fused` do not wrap a Reader that one of them made: they extend its chain -- ConvertReader ->
// ShiftReader -> Gain -> Multiply -> DecimateReader / DownsampleReader / ConvolutionReader collapse into one
// hzsdr_chain, one launch per slot -- and the Reader reads AHEAD: `readahead` Reader blocks of 32 Ki samples per slot of a
// pinned ring.  What the nest means is kept: the same samples bit for bit, block-structured stages hand out whole
// blocks only (a source that ends inside a block loses that partial block, as ReadFull's ErrUnexpectedEOF does in
// read_transformer.go:120-135), pass-through stages hand out whatever the source delivered, the source's error is
// sticky and surfaces behind everything read before it.
class ChainReader : public Reader {
public:
    struct Stage { int kind; double shift; float gain, re, im; };  // 0 Shift, 1 Gain, 2 Multiply
    ChainReader(const Context &x, ReaderPtr src, int readahead) : x_(x), src_(std::move(src)), readahead_(readahead) {
        src_format_ = src_->SampleFormat();
        rate_ = src_->SampleRate();
    }
    bool open() const { return !chain_ && term_ == 0; }
    bool c64_here() const { return src_format_ == HZSDR_FMT_C64 || converted_; }
    bool extend_convert(int to) {
        if (!open() || to != HZSDR_FMT_C64 || !stages_.empty() || src_format_ == HZSDR_FMT_C64 || converted_) return false;
        converted_ = true;
        block_ = lcm(block_, kBlock);
        return true;
    }
    bool extend_stage(const Stage &st) {
        if (!open() || !c64_here()) return false;
        stages_.push_back(st);
        return true;
    }
    // the north-star terminal (kind 4: an N-tap FIR whose output is kept every `factor` samples -- hzsdr_chain_fir_decimate;
    // the reference has no such Reader): `slots` slots in the pinned ring, `group` of them per call of the chain
    bool extend_fir(const std::vector<std::complex<float>> &taps, unsigned factor, int slots, int group) {
        if (!open()) return false;
        if (!c64_here()) converted_ = true;  // (the terminal converts on its way in, as DownsampleReader does)
        term_ = 4, factor_ = factor, taps_ = taps;
        block_ = lcm(block_, factor);
        rate_ /= factor;
        slots_ = std::max(2, slots);
        group_ = std::max(1, std::min(std::min(group, 8), slots_ - 1));
        return true;
    }
    const Chain *chain() const { return chain_.get(); }
    // kind 1 Decimate, 2 Downsample (its own conversion of a raw source included), 3 Convolution
    bool extend_terminal(int kind, unsigned factor, Samples filter, size_t block) {
        if (chain_) return false;
        if (kind == 1 && term_ == 3 && decimate_ == 1 && kBlock % filter_.size() == 0) {  // DecimateReader behind the ConvolutionReader
            decimate_ = factor;
            block_ = lcm(block_, kBlock);
            rate_ /= factor;
            return true;
        }
        if (kind == 2 && open() && !c64_here() && stages_.empty()) converted_ = true;
        if (!open() || !c64_here()) return false;
        term_ = kind, factor_ = factor;
        if (kind == 3) filter_.assign((const std::complex<float> *)filter.data, (const std::complex<float> *)filter.data + filter.length);
        block_ = lcm(block_, block);
        if (kind == 1 || kind == 2) rate_ /= factor;
        return true;
    }
    int SampleFormat() const override { return c64_here() ? HZSDR_FMT_C64 : src_format_; }
    unsigned SampleRate() const override { return rate_; }
    size_t Read(Samples s) override {
        if (s.format != SampleFormat() || s.format != HZSDR_FMT_C64) throw Error(HZSDR_ERR_FORMAT_MISMATCH, hzsdr_strerror(HZSDR_ERR_FORMAT_MISMATCH));
        if (!chain_) build();
        if (off_ >= pending_.length) {
            // everything but the slot being consumed is in flight -- refilled `group_` slots at a time, ONE call of the chain
            // per group (hzsdr_ring_submit_many): a refill waits until that many slots are free, or nothing is in flight
            for (;;) {
                const int free_slots = slots_ - 1 - inflight_;
                if (free_slots < 1 || (free_slots < group_ && inflight_ > 0)) break;
                if (fill(std::min(group_, free_slots)) == 0) break;
            }
            if (inflight_ == 0) {
                if (err_) std::rethrow_exception(err_);
                throw Eof();
            }
            pending_ = ring_->Pop();
            inflight_--;
            off_ = 0;
            if (pending_.length == 0) return 0;
        }
        const size_t n = std::min(pending_.length - off_, s.length);
        memcpy(s.data, (const char *)pending_.data + 8 * off_, 8 * n);
        off_ += n;
        return n;
    }

private:
    static constexpr size_t kBlock = 32 * 1024;
    static size_t gcd(size_t a, size_t b) { while (b) { const size_t t = a % b; a = b; b = t; } return a; }
    static size_t lcm(size_t a, size_t b) { return a / gcd(a, b) * b; }
    void build() {
        chain_ = std::make_unique<Chain>(x_, src_format_, src_->SampleRate());
        for (const Stage &st : stages_) {
            if (st.kind == 0) chain_->Shift(st.shift);
            else if (st.kind == 1) chain_->Gain(st.gain);
            else chain_->Multiply(st.re, st.im);
        }
        if (term_ == 1) chain_->Decimate(factor_);
        else if (term_ == 2) chain_->Downsample(factor_);
        else if (term_ == 3) chain_->Convolution(Samples{HZSDR_FMT_C64, filter_.data(), filter_.size()}, decimate_);
        else if (term_ == 4) {
            chain_->FirDecimate(taps_, factor_);
            check(x_.raw(), hzsdr_chain_pipeline(chain_->raw(), 1));  // (consecutive calls overlap: the ring says what each call's buffers wait for)
        }
        const size_t unit = block_ > 1 ? block_ : kBlock;
        slot_len_ = std::max<size_t>(1, (size_t)readahead_ * kBlock / unit) * unit;
        ring_ = std::make_unique<Ring>(*chain_, slot_len_, slots_);
    }
    // Read the source into up to `want` slots and submit them: the full ones together, ONE call of the chain, a short last
    // one (the source ended) by itself.  -> slots submitted.  An acquired slot is submitted or released whatever the
    // source throws (the error is sticky and surfaces behind everything read before it).
    int fill(int want) {
        if (err_) return 0;
        int first = -1, full = 0, done = 0;
        auto flush = [&]() {
            if (full) {
                ring_->SubmitMany(first, full, slot_len_);
                inflight_ += full;
                full = 0;
            }
        };
        while (done < want && !err_) {
            int slot = -1;
            Samples iq = ring_->Acquire(src_format_, &slot);
            size_t n = 0;
            int idle = 0;
            try {
                while (n < slot_len_) {
                    const size_t got = src_->Read(iq.slice(n, slot_len_));
                    n += got;
                    idle = got ? 0 : idle + 1;
                    if (idle >= 100) throw Error(HZSDR_ERR_INVALID_ARGUMENT, "multiple Read calls return no data or error");  // io.ErrNoProgress
                }
            } catch (...) {
                err_ = std::current_exception();
            }
            n = n / block_ * block_;
            if (n == slot_len_) {
                if (first < 0 || full == 0) first = slot;
                full++, done++;
                continue;
            }
            flush();
            if (n == 0) {
                ring_->Release(slot);
            } else {
                ring_->Submit(slot, n);
                inflight_++, done++;
            }
            return done;
        }
        flush();
        return done;
    }
    const Context &x_;
    ReaderPtr src_;
    int readahead_, src_format_ = 0;
    unsigned rate_ = 0;
    bool converted_ = false;
    std::vector<Stage> stages_;
    int term_ = 0;
    unsigned factor_ = 1, decimate_ = 1;
    std::vector<std::complex<float>> filter_, taps_;
    int slots_ = 3, group_ = 1;
    size_t block_ = 1, slot_len_ = 0;
    std::unique_ptr<Chain> chain_;
    std::unique_ptr<Ring> ring_;
    Samples pending_{};
    size_t off_ = 0;
    int inflight_ = 0;
    std::exception_ptr err_;
};

// The constructor set that fuses (go/hip: Context.Readers()); every name falls back to the plain constructor above when
// the stage cannot join a chain.
struct Fused {
    const Context &x;
    int readahead = 32;
    template <class How> std::shared_ptr<ChainReader> fused(ReaderPtr r, How how) const {
        if (auto cr = std::dynamic_pointer_cast<ChainReader>(r)) {
            if (how(*cr)) return cr;
        }
        auto cr = std::make_shared<ChainReader>(x, r, readahead);
        if (how(*cr)) return cr;
        return nullptr;
    }
    ReaderPtr ConvertReader(ReaderPtr in, int to) const {
        if (auto f = fused(in, [&](ChainReader &c) { return c.extend_convert(to); })) return f;
        return stream::ConvertReader(x, std::move(in), to);
    }
    ReaderPtr ShiftReader(ReaderPtr r, double hz) const {
        if (r->SampleFormat() != HZSDR_FMT_C64) throw Error(HZSDR_ERR_FORMAT_UNKNOWN, hzsdr_strerror(HZSDR_ERR_FORMAT_UNKNOWN));
        if (auto f = fused(r, [&](ChainReader &c) { return c.extend_stage({0, hz, 0.f, 0.f, 0.f}); })) return f;
        return stream::ShiftReader(x, std::move(r), hz);
    }
    ReaderPtr Gain(ReaderPtr r, float v) const {
        if (r->SampleFormat() == HZSDR_FMT_C64)
            if (auto f = fused(r, [&](ChainReader &c) { return c.extend_stage({1, 0.0, v, 0.f, 0.f}); })) return f;
        return stream::Gain(x, std::move(r), v);
    }
    ReaderPtr Multiply(ReaderPtr r, float re, float im) const {
        if (r->SampleFormat() == HZSDR_FMT_C64 && !(re == 1.0f && im == 0.0f))
            if (auto f = fused(r, [&](ChainReader &c) { return c.extend_stage({2, 0.0, 0.f, re, im}); })) return f;
        return stream::Multiply(x, std::move(r), re, im);
    }
    ReaderPtr DecimateReader(ReaderPtr in, unsigned factor) const {
        if (in->SampleFormat() == HZSDR_FMT_C64 && factor > 0)
            if (auto f = fused(in, [&](ChainReader &c) { return c.extend_terminal(1, factor, Samples{}, 32 * 1024); })) return f;
        return stream::DecimateReader(x, std::move(in), factor);
    }
    ReaderPtr DownsampleReader(ReaderPtr in, unsigned factor) const {
        const int f0 = in->SampleFormat();
        if ((f0 == HZSDR_FMT_C64 || f0 == HZSDR_FMT_U8 || f0 == HZSDR_FMT_I16) && factor > 0)
            if (auto f = fused(in, [&](ChainReader &c) { return c.extend_terminal(2, factor, Samples{}, 32 * 1024); })) return f;
        return stream::DownsampleReader(x, std::move(in), factor);
    }
    ReaderPtr ConvolutionReader(ReaderPtr r, Samples filter) const {
        if (r->SampleFormat() != HZSDR_FMT_C64) throw Error(HZSDR_ERR_FORMAT_UNKNOWN, hzsdr_strerror(HZSDR_ERR_FORMAT_UNKNOWN));
        if (auto f = fused(r, [&](ChainReader &c) { return c.extend_terminal(3, 1, filter, filter.length); })) return f;
        return stream::ConvolutionReader(x, std::move(r), filter);
    }
    // The north-star terminal as a Reader (BASELINE.json north_star; the reference's Downsample is the boxcar,
    // stream/downsample.go:47-64, so name and signature follow DecimateReader's, stream/decimate.go:34): always fused --
    // ConvertReader / ShiftReader / Gain / Multiply in front of it join its chain -- `slots` slots in the pinned ring,
    // `group` of them per call of the chain (hzsdr_ring_submit_many: one launch of the int8 matrix kernel per group).
    std::shared_ptr<ChainReader> FirDecimateReader(ReaderPtr in, const std::vector<std::complex<float>> &taps, unsigned factor, int slots = 5,
                                                   int group = 4) const {
        auto f = fused(in, [&](ChainReader &c) { return c.extend_fir(taps, factor, slots, group); });
        if (!f) throw Error(HZSDR_ERR_INVALID_ARGUMENT, "FirDecimateReader: the stage does not fit the Reader in front of it");
        return f;
    }
};

}  // namespace stream

namespace fft {
// The fused power spectrum (include/hzsdr_spectrum.h): Push consumes every sample it is given and returns the rows
// that complete, rows x n float32, row-major, in the spectrum's fft.Order (fft/result.go:34-47).
class Spectrum {
public:
    Spectrum(const Context &x, int src_format, size_t n, size_t hop, size_t avg, const std::vector<float> &window, float scale,
             int order = HZSDR_ORDER_NEGATIVE_FIRST, bool db = false)
        : x_(x), n_(n) {
        check(x_.raw(), hzsdr_spectrum_create(x_.raw(), src_format, n, hop, avg, window.empty() ? nullptr : window.data(), scale,
                                              order, db ? HZSDR_SPECTRUM_DB : HZSDR_SPECTRUM_POWER, &s_));
    }
    ~Spectrum() { if (s_) hzsdr_spectrum_free(s_); }
    Spectrum(const Spectrum &) = delete;
    Spectrum &operator=(const Spectrum &) = delete;
    size_t RowsFor(size_t n_in) const {
        size_t r = 0;
        check(x_.raw(), hzsdr_spectrum_rows_for(s_, n_in, &r));
        return r;
    }
    // (a HOST context's buffers: the rows come back in a vector)
    std::vector<float> Push(Samples in) {
        std::vector<float> out(RowsFor(in.length) * n_);
        size_t rows = 0;
        check(x_.raw(), hzsdr_spectrum_push(s_, in.data, in.length, out.empty() ? nullptr : out.data(), out.size() / n_, &rows));
        out.resize(rows * n_);
        return out;
    }
    // -> (frames summed into the open row, samples held for the next frame)
    std::pair<size_t, size_t> Pending() const {
        size_t f = 0, h = 0;
        check(x_.raw(), hzsdr_spectrum_pending(s_, &f, &h));
        return {f, h};
    }
    Spectrum &Options(int form) { check(x_.raw(), hzsdr_spectrum_options(s_, form)); return *this; }
    int LastForm() const {
        int f = 0;
        check(x_.raw(), hzsdr_spectrum_last_form(s_, &f));
        return f;
    }
    void Reset() { check(x_.raw(), hzsdr_spectrum_reset(s_)); }
    size_t Bins() const { return n_; }

private:
    const Context &x_;
    size_t n_;
    hzsdr_spectrum *s_ = nullptr;
};

// What the three polyphase bank classes below share: the handle and its life, Pending, Reset and Channels.  H is the
// handle, the rest hzsdr_<bank>_pending, _reset and _free.
template <class H, auto PendingFn, auto ResetFn, auto FreeFn>
class PolyphaseBank {
public:
    PolyphaseBank(const PolyphaseBank &) = delete;
    PolyphaseBank &operator=(const PolyphaseBank &) = delete;
    // -> (samples held for the next frame -- the synthesis bank: partial sums held behind the samples written --, index
    // of the next frame)
    std::pair<size_t, uint64_t> Pending() const {
        size_t h = 0;
        uint64_t j = 0;
        check(x_.raw(), PendingFn(h_, &h, &j));
        return {h, j};
    }
    void Reset() { check(x_.raw(), ResetFn(h_)); }
    size_t Channels() const { return m_; }

protected:
    PolyphaseBank(const Context &x, size_t channels) : x_(x), m_(channels) {}
    ~PolyphaseBank() { if (h_) FreeFn(h_); }
    const Context &x_;
    size_t m_;
    H *h_ = nullptr;
};
// ... and the two analysis banks on top of it: the create, FramesFor and Push, over hzsdr_<bank>_create, _frames_for and
// _push.
template <class H, auto CreateFn, auto FramesForFn, auto PushFn, auto PendingFn, auto ResetFn, auto FreeFn>
class AnalysisBank : public PolyphaseBank<H, PendingFn, ResetFn, FreeFn> {
public:
    size_t FramesFor(size_t n_in) const {
        size_t f = 0;
        check(this->x_.raw(), FramesForFn(this->h_, n_in, &f));
        return f;
    }
    // (a HOST context's buffers: the frames come back in a vector)
    std::vector<std::complex<float>> Push(Samples in) {
        const size_t want = FramesFor(in.length);
        std::vector<std::complex<float>> out(want * this->m_);
        size_t frames = 0;
        check(this->x_.raw(), PushFn(this->h_, in.data, in.length, out.empty() ? nullptr : out.data(), want, want, &frames));
        return out;
    }

protected:
    AnalysisBank(const Context &x, int src_format, size_t channels, const std::vector<float> &taps, size_t hop, int order, int layout)
        : PolyphaseBank<H, PendingFn, ResetFn, FreeFn>(x, channels) {
        check(x.raw(), CreateFn(x.raw(), src_format, channels, taps.empty() ? nullptr : taps.data(), taps.size(), hop, order, layout, &this->h_));
    }
};

// The polyphase channelizer (include/hzsdr_channelizer.h): Push consumes every sample it is given and returns the
// frames that complete as complex64, frames x channels (HZSDR_CHANNELIZER_FRAME_MAJOR) or channels x frames
// (HZSDR_CHANNELIZER_CHANNEL_MAJOR, the pitch being the frames of the push), in the channelizer's fft.Order
// (fft/result.go:34-47).
class Channelizer : public AnalysisBank<hzsdr_channelizer, hzsdr_channelizer_create, hzsdr_channelizer_frames_for, hzsdr_channelizer_push,
                                        hzsdr_channelizer_pending, hzsdr_channelizer_reset, hzsdr_channelizer_free> {
public:
    Channelizer(const Context &x, int src_format, size_t channels, const std::vector<float> &taps, size_t hop,
                int order = HZSDR_ORDER_NEGATIVE_FIRST, int layout = HZSDR_CHANNELIZER_FRAME_MAJOR)
        : AnalysisBank(x, src_format, channels, taps, hop, order, layout) {}
};
// The channel bank (include/hzsdr_chanbank.h): the polyphase channelizer for the small channel counts, any `channels`
// from 2 to 255.  Push consumes every sample it is given and returns the frames that complete as complex64, frames x
// channels (HZSDR_CHANNELIZER_FRAME_MAJOR) or channels x frames (HZSDR_CHANNELIZER_CHANNEL_MAJOR, the pitch being the
// frames of the push); HZSDR_ORDER_NEGATIVE_FIRST is ascending signed frequency, position 0 at -floor(channels / 2).
class ChannelBank : public AnalysisBank<hzsdr_chanbank, hzsdr_chanbank_create, hzsdr_chanbank_frames_for, hzsdr_chanbank_push, hzsdr_chanbank_pending,
                                        hzsdr_chanbank_reset, hzsdr_chanbank_free> {
public:
    ChannelBank(const Context &x, int src_format, size_t channels, const std::vector<float> &taps, size_t hop,
                int order = HZSDR_ORDER_NEGATIVE_FIRST, int layout = HZSDR_CHANNELIZER_FRAME_MAJOR)
        : AnalysisBank(x, src_format, channels, taps, hop, order, layout), l_(taps.size()) {}
    // -> (frames per workgroup, rows of the real matrix per workgroup, HZSDR_CHANBANK_FORM_*)
    std::tuple<size_t, size_t, int> Plan() const {
        size_t t = 0, r = 0;
        int f = 0;
        check(x_.raw(), hzsdr_chanbank_plan(h_, &t, &r, &f));
        return {t, r, f};
    }
    // row k of the DFT table: the channels rounded up to an even count of complex64 values
    std::vector<std::complex<float>> Table(size_t k) const {
        std::vector<std::complex<float>> out((m_ + 1) & ~(size_t)1);
        check(x_.raw(), hzsdr_chanbank_readout(h_, HZSDR_CHANBANK_READ_DFT, k, out.data(), out.size()));
        return out;
    }
    std::vector<float> Taps() const {
        std::vector<float> out(l_);
        check(x_.raw(), hzsdr_chanbank_readout(h_, HZSDR_CHANBANK_READ_TAPS, 0, out.data(), out.size()));
        return out;
    }

private:
    size_t l_;
};
// The polyphase synthesis bank (include/hzsdr_synthesizer.h), the channelizer's adjoint: Push consumes frames of
// `channels` complex64 values, frames x channels (HZSDR_CHANNELIZER_FRAME_MAJOR) or channels x frames
// (HZSDR_CHANNELIZER_CHANNEL_MAJOR, the pitch being the frames of the push), in the synthesizer's fft.Order
// (fft/result.go:34-47), and returns the frames * hop samples they complete in the destination format; Flush returns
// the stream's tail and starts over.
class Synthesizer : public PolyphaseBank<hzsdr_synthesizer, hzsdr_synthesizer_pending, hzsdr_synthesizer_reset, hzsdr_synthesizer_free> {
public:
    Synthesizer(const Context &x, int dst_format, size_t channels, const std::vector<float> &taps, size_t hop,
                int order = HZSDR_ORDER_NEGATIVE_FIRST, int layout = HZSDR_CHANNELIZER_FRAME_MAJOR)
        : PolyphaseBank(x, channels), fmt_(dst_format), hop_(hop) {
        check(x_.raw(), hzsdr_synthesizer_create(x_.raw(), dst_format, channels, taps.empty() ? nullptr : taps.data(), taps.size(), hop,
                                                 order, layout, &h_));
    }
    // (a HOST context's buffers: the samples come back in a Buffer of the destination format)
    Buffer Push(const std::vector<std::complex<float>> &frames) {
        const size_t f = frames.size() / m_;
        Buffer out(fmt_, f * hop_);
        size_t n = 0;
        check(x_.raw(), hzsdr_synthesizer_push(h_, frames.empty() ? nullptr : frames.data(), f, f, out.view.length ? out.view.data : nullptr,
                                               out.view.length, &n));
        return out;
    }
    Buffer Flush() {
        Buffer out(fmt_, Pending().first);
        size_t n = 0;
        check(x_.raw(), hzsdr_synthesizer_flush(h_, out.view.length ? out.view.data : nullptr, out.view.length, &n));
        return out;
    }
    size_t GroupFrames() const {
        size_t f = 0;
        check(x_.raw(), hzsdr_synthesizer_group_frames(h_, &f));
        return f;
    }

private:
    int fmt_;
    size_t hop_;
};
}  // namespace fft

namespace stream {
// The polyphase rational resampler (include/hzsdr_resampler.h): `streams` rows of src_format samples at up/down times
// their rate, complex64, scipy.signal.upfirdn's definition.  Push consumes `n` samples of every row (row s starts
// s * in_stride samples into `in`; dense rows when in_stride is 0) and returns the outputs they complete, dense rows of
// the returned count; Flush returns the outputs that still depend on samples pushed and starts over.
class Resampler {
public:
    Resampler(const Context &x, int src_format, size_t up, size_t down, const std::vector<float> &taps, size_t streams = 1)
        : x_(x), streams_(streams) {
        check(x_.raw(), hzsdr_resampler_create(x_.raw(), src_format, up, down, taps.empty() ? nullptr : taps.data(), taps.size(), streams, &r_));
    }
    ~Resampler() { if (r_) hzsdr_resampler_free(r_); }
    Resampler(const Resampler &) = delete;
    Resampler &operator=(const Resampler &) = delete;
    // (a HOST context's buffers: view.length is streams * count, row s at s * count)
    Buffer Push(const void *in, size_t n, size_t in_stride = 0) {
        const size_t count = OutputsFor(n);
        Buffer out(HZSDR_FMT_C64, streams_ * count);
        size_t w = 0;
        check(x_.raw(), hzsdr_resampler_push(r_, n ? in : nullptr, n, in_stride ? in_stride : n, count ? out.view.data : nullptr, count, count, &w));
        return out;
    }
    Buffer Flush() {
        const size_t count = std::get<2>(Pending());
        Buffer out(HZSDR_FMT_C64, streams_ * count);
        size_t w = 0;
        check(x_.raw(), hzsdr_resampler_flush(r_, count ? out.view.data : nullptr, count, count, &w));
        return out;
    }
    size_t OutputsFor(size_t n) const {
        size_t c = 0;
        check(x_.raw(), hzsdr_resampler_outputs_for(r_, n, &c));
        return c;
    }
    // -> (samples consumed, index of the next output, outputs a flush would write now), per stream
    std::tuple<uint64_t, uint64_t, size_t> Pending() const {
        uint64_t n = 0, m = 0;
        size_t f = 0;
        check(x_.raw(), hzsdr_resampler_pending(r_, &n, &m, &f));
        return {n, m, f};
    }
    // -> (outputs per workgroup, HZSDR_RESAMPLER_FORM_*)
    std::pair<size_t, int> Plan() const {
        size_t t = 0;
        int f = 0;
        check(x_.raw(), hzsdr_resampler_plan(r_, &t, &f));
        return {t, f};
    }
    void Reset() { check(x_.raw(), hzsdr_resampler_reset(r_)); }
    size_t Streams() const { return streams_; }

private:
    const Context &x_;
    size_t streams_;
    hzsdr_resampler *r_ = nullptr;
};

// The demodulator bank (include/hzsdr_demod.h): HZSDR_DEMOD_FM, _PHASE, _ENVELOPE or _POWER of `streams` rows of
// src_format samples, then the real post-filter `taps` (empty: [1.0], the bare detector) and a decimation by `down`;
// real float32.  Push consumes `n` samples of every row (row s starts s * in_stride samples into `in`; dense rows when
// in_stride is 0) and returns the outputs they complete, dense rows of the returned count; Flush returns the outputs
// that still depend on samples pushed and starts over.
class Demodulator {
public:
    Demodulator(const Context &x, int src_format, int mode, const std::vector<float> &taps = {}, size_t down = 1, size_t streams = 1)
        : x_(x), streams_(streams) {
        const float one = 1.0f;
        check(x_.raw(), hzsdr_demod_create(x_.raw(), src_format, mode, down, taps.empty() ? &one : taps.data(), taps.empty() ? 1 : taps.size(),
                                           streams, &d_));
    }
    ~Demodulator() { if (d_) hzsdr_demod_free(d_); }
    Demodulator(const Demodulator &) = delete;
    Demodulator &operator=(const Demodulator &) = delete;
    // (row s of the result is [s * count, (s + 1) * count) with count = size() / Streams())
    std::vector<float> Push(const void *in, size_t n, size_t in_stride = 0) {
        const size_t count = OutputsFor(n);
        std::vector<float> out(streams_ * count);
        size_t w = 0;
        check(x_.raw(), hzsdr_demod_push(d_, n ? in : nullptr, n, in_stride ? in_stride : n, count ? out.data() : nullptr, count, count, &w));
        return out;
    }
    std::vector<float> Flush() {
        const size_t count = std::get<2>(Pending());
        std::vector<float> out(streams_ * count);
        size_t w = 0;
        check(x_.raw(), hzsdr_demod_flush(d_, count ? out.data() : nullptr, count, count, &w));
        return out;
    }
    size_t OutputsFor(size_t n) const {
        size_t c = 0;
        check(x_.raw(), hzsdr_demod_outputs_for(d_, n, &c));
        return c;
    }
    // -> (samples consumed, index of the next output, outputs a flush would write now), per stream
    std::tuple<uint64_t, uint64_t, size_t> Pending() const {
        uint64_t n = 0, m = 0;
        size_t f = 0;
        check(x_.raw(), hzsdr_demod_pending(d_, &n, &m, &f));
        return {n, m, f};
    }
    // -> (outputs per workgroup, HZSDR_DEMOD_FORM_*)
    std::pair<size_t, int> Plan() const {
        size_t t = 0;
        int f = 0;
        check(x_.raw(), hzsdr_demod_plan(d_, &t, &f));
        return {t, f};
    }
    void Reset() { check(x_.raw(), hzsdr_demod_reset(d_)); }
    size_t Streams() const { return streams_; }

private:
    const Context &x_;
    size_t streams_;
    hzsdr_demod *d_ = nullptr;
};

// What the four row-wave bank classes below share: the handle and its life, and the calls that differ from bank to bank
// only in the C function's name.  H is the handle, Z a word of the state; the functions are hzsdr_<bank>_free, _position,
// _plan, _reset, _get_state and _set_state.  State() is the bank's state array as its header lays it out, SetState() puts
// one back, Plan() is (rows per wave, samples per tile, HZSDR_<BANK>_FORM_*).
template <class H, class Z, auto Free, auto PositionFn, auto PlanFn, auto ResetFn, auto GetState, auto SetStateFn>
class RowWaveBank {
public:
    RowWaveBank(const RowWaveBank &) = delete;
    RowWaveBank &operator=(const RowWaveBank &) = delete;
    std::vector<Z> State() const {
        std::vector<Z> z(state_words_);
        check(x_.raw(), GetState(h_, z.data(), z.size()));
        return z;
    }
    void SetState(const std::vector<Z> &z, uint64_t position = 0) { check(x_.raw(), SetStateFn(h_, z.data(), z.size(), position)); }
    uint64_t Position() const {
        uint64_t p = 0;
        check(x_.raw(), PositionFn(h_, &p));
        return p;
    }
    std::tuple<size_t, size_t, int> Plan() const {
        size_t g = 0, t = 0;
        int f = 0;
        check(x_.raw(), PlanFn(h_, &g, &t, &f));
        return {g, t, f};
    }
    void Reset() { check(x_.raw(), ResetFn(h_)); }
    size_t Rows() const { return rows_; }

protected:
    RowWaveBank(const Context &x, size_t rows, size_t state_words = 0) : x_(x), rows_(rows), state_words_(state_words) {}
    ~RowWaveBank() { if (h_) Free(h_); }
    // one output per input and, where `track` is given, dense rows of n track values (Push: hzsdr_<bank>_push)
    template <auto Push, typename S> std::vector<S> push_tracked(const void *in, size_t n, size_t in_stride, std::vector<float> *track) {
        std::vector<S> out(rows_ * n);
        if (track) track->assign(rows_ * n, 0.0f);
        check(x_.raw(), Push(h_, n ? in : nullptr, n, in_stride ? in_stride : n, n ? out.data() : nullptr, n, track && n ? track->data() : nullptr, n));
        return out;
    }
    template <auto Push> void push_in_place(void *rows, size_t n, size_t pitch) {
        check(x_.raw(), Push(h_, n ? rows : nullptr, n, pitch ? pitch : n, n ? rows : nullptr, pitch ? pitch : n, nullptr, 0));
    }
    const Context &x_;
    size_t rows_, state_words_;
    H *h_ = nullptr;
};

// The IIR bank (include/hzsdr_iir.h): the cascade `sections` -- (b0, b1, b2, a1, a2) per section, one cascade shared by
// all rows, or rows of them when per_row -- over `rows` rows of HZSDR_IIR_REAL_F32 samples (float32 out: Push) or of a
// source format (complex64 out: PushComplex).  Push filters `n` samples of every row (row r starts r * in_stride
// samples into `in`; dense rows when in_stride is 0) and returns dense rows of n; one output per input, no flush.
// The state: row, section, z1 / z2, re / im.
class IirBank : public RowWaveBank<hzsdr_iir, float, hzsdr_iir_free, hzsdr_iir_position, hzsdr_iir_plan, hzsdr_iir_reset, hzsdr_iir_get_state,
                                   hzsdr_iir_set_state> {
public:
    IirBank(const Context &x, int kind_or_format, const std::vector<float> &sections, size_t rows = 1, bool per_row = false)
        : RowWaveBank(x, rows), complex_(kind_or_format != HZSDR_IIR_REAL_F32) {
        const size_t per = 5 * (per_row && rows ? rows : 1);
        sections_ = sections.size() / per;
        if (sections_ * per != sections.size()) throw std::invalid_argument("IirBank: sections are S * 5, or rows * S * 5 values");
        state_words_ = rows_ * sections_ * 2 * (complex_ ? 2 : 1);
        check(x_.raw(), hzsdr_iir_create(x_.raw(), kind_or_format, sections.data(), sections_, per_row ? 1 : 0, rows, &h_));
    }
    // real rows (row r of the result is [r * n, (r + 1) * n))
    std::vector<float> Push(const void *in, size_t n, size_t in_stride = 0) {
        if (complex_) throw std::invalid_argument("IirBank: complex rows go through PushComplex");
        return push<float>(in, n, in_stride);
    }
    std::vector<std::complex<float>> PushComplex(const void *in, size_t n, size_t in_stride = 0) {
        if (!complex_) throw std::invalid_argument("IirBank: real rows go through Push");
        return push<std::complex<float>>(in, n, in_stride);
    }
    // the same count and form; the state and the position stay
    void SetSections(const std::vector<float> &sections) {
        if (sections.size() % 5) throw std::invalid_argument("IirBank: sections are S * 5, or rows * S * 5 values");
        check(x_.raw(), hzsdr_iir_set_sections(h_, sections.data(), sections_));
    }
    size_t Sections() const { return sections_; }

private:
    template <class V> std::vector<V> push(const void *in, size_t n, size_t in_stride) {
        std::vector<V> out(rows_ * n);
        size_t w = 0;
        check(x_.raw(), hzsdr_iir_push(h_, n ? in : nullptr, n, in_stride ? in_stride : n, n ? out.data() : nullptr, n, n, &w));
        return out;
    }
    size_t sections_ = 0;
    bool complex_;
};

// The symbol-timing recovery bank (include/hzsdr_symsync.h): a Gardner loop around a cubic interpolator over `rows` rows
// of HZSDR_SYMSYNC_REAL_F32 samples (float32 symbols: Push) or HZSDR_FMT_C64 ones (complex64 symbols: PushComplex), with
// the parameters sps, limit, g_mu, g_omega shared by all rows, or rows of them when per_row.  Push runs `n` samples of
// every row (row r starts r * in_stride samples into `in`; dense rows when in_stride is 0) and returns the rows' symbols,
// each row cut to its own count; nothing to flush.  The state: per row c, h, flag, y_prev, y_mid, x1, x2, x3.
class SymbolSync : public RowWaveBank<hzsdr_symsync, float, hzsdr_symsync_free, hzsdr_symsync_position, hzsdr_symsync_plan, hzsdr_symsync_reset,
                                      hzsdr_symsync_get_state, hzsdr_symsync_set_state> {
public:
    SymbolSync(const Context &x, int kind, const std::vector<float> &params, size_t rows = 1, bool per_row = false)
        : RowWaveBank(x, rows, rows * (kind != HZSDR_SYMSYNC_REAL_F32 ? 13 : 8)), complex_(kind != HZSDR_SYMSYNC_REAL_F32) {
        if (params.size() != 4 * (per_row ? rows : 1)) throw std::invalid_argument("SymbolSync: params are 4, or rows * 4 values");
        check(x_.raw(), hzsdr_symsync_create(x_.raw(), kind, params.data(), per_row ? 1 : 0, rows, &h_));
    }
    std::vector<std::vector<float>> Push(const void *in, size_t n, size_t in_stride = 0) {
        if (complex_) throw std::invalid_argument("SymbolSync: complex rows go through PushComplex");
        return push<float>(in, n, in_stride);
    }
    std::vector<std::vector<std::complex<float>>> PushComplex(const void *in, size_t n, size_t in_stride = 0) {
        if (!complex_) throw std::invalid_argument("SymbolSync: real rows go through Push");
        return push<std::complex<float>>(in, n, in_stride);
    }
    size_t MaxSymbols(size_t n) const {
        size_t b = 0;
        check(x_.raw(), hzsdr_symsync_max_symbols(h_, n, &b));
        return b;
    }
    // the same form; the state and the position stay
    void SetParams(const std::vector<float> &params) { check(x_.raw(), hzsdr_symsync_set_params(h_, params.data())); }

private:
    template <class V> std::vector<std::vector<V>> push(const void *in, size_t n, size_t in_stride) {
        const size_t bound = MaxSymbols(n);
        std::vector<V> out(rows_ * bound);
        std::vector<uint32_t> counts(rows_, 0);
        size_t most = 0;
        check(x_.raw(), hzsdr_symsync_push(h_, n ? in : nullptr, n, in_stride ? in_stride : n, bound ? out.data() : nullptr, bound, bound, counts.data(), &most));
        std::vector<std::vector<V>> rows(rows_);
        for (size_t r = 0; r < rows_; r++) rows[r].assign(out.begin() + r * bound, out.begin() + r * bound + counts[r]);
        return rows;
    }
    bool complex_;
};

// The carrier recovery bank (include/hzsdr_carrier.h): a second-order loop around a numerically controlled oscillator over
// `rows` complex64 rows, with the detector `mode` (HZSDR_CARRIER_TONE, _BPSK, _QPSK) and the parameters alpha, beta, f0,
// fmin, fmax shared by all rows, or rows of them when per_row.  Push runs `n` samples of every row (row r starts
// r * in_stride samples into `in`; dense rows when in_stride is 0) and returns dense rows of n derotated samples; where
// `track` is given it takes dense rows of n frequency estimates, in cycles per sample.  One output per input, no flush.
// The state: per row theta, F.
class CarrierLoop : public RowWaveBank<hzsdr_carrier, uint32_t, hzsdr_carrier_free, hzsdr_carrier_position, hzsdr_carrier_plan, hzsdr_carrier_reset,
                                       hzsdr_carrier_get_state, hzsdr_carrier_set_state> {
public:
    CarrierLoop(const Context &x, int mode, const std::vector<float> &params, size_t rows = 1, bool per_row = false) : RowWaveBank(x, rows, rows * 2) {
        if (params.size() != 5 * (per_row ? rows : 1)) throw std::invalid_argument("CarrierLoop: params are 5, or rows * 5 values");
        check(x_.raw(), hzsdr_carrier_create(x_.raw(), mode, params.data(), per_row ? 1 : 0, rows, &h_));
    }
    std::vector<std::complex<float>> Push(const void *in, size_t n, size_t in_stride = 0, std::vector<float> *track = nullptr) {
        return push_tracked<hzsdr_carrier_push, std::complex<float>>(in, n, in_stride, track);
    }
    // the rows derotated where they lie (pitch: samples from one row's start to the next; n when 0)
    void PushInPlace(std::complex<float> *rows, size_t n, size_t pitch = 0) { push_in_place<hzsdr_carrier_push>(rows, n, pitch); }
    // the same form; theta, F and the position stay
    void SetParams(const std::vector<float> &params) { check(x_.raw(), hzsdr_carrier_set_params(h_, params.data())); }
};

// The AGC bank (include/hzsdr_agc.h): a multiplicative gain loop over `rows` rows of `kind` (HZSDR_AGC_REAL_F32: float
// rows; HZSDR_FMT_C64: std::complex<float> rows), with the parameters ref, attack, decay, floor, g0, gmin, gmax shared by
// all rows, or rows of them when per_row.  Push runs `n` samples of every row (row r starts r * in_stride samples into
// `in`; dense rows when in_stride is 0) and returns dense rows of n levelled samples of the input's type (S is float or
// std::complex<float>, as the kind says); where `track` is given it takes dense rows of n applied gains.  One output per
// input, no flush.  The state: per row the gain; ref / gain is the row's level.
class Agc : public RowWaveBank<hzsdr_agc, float, hzsdr_agc_free, hzsdr_agc_position, hzsdr_agc_plan, hzsdr_agc_reset, hzsdr_agc_get_state,
                               hzsdr_agc_set_state> {
public:
    Agc(const Context &x, int kind, const std::vector<float> &params, size_t rows = 1, bool per_row = false) : RowWaveBank(x, rows, rows), kind_(kind) {
        if (params.size() != 7 * (per_row ? rows : 1)) throw std::invalid_argument("Agc: params are 7, or rows * 7 values");
        check(x_.raw(), hzsdr_agc_create(x_.raw(), kind, params.data(), per_row ? 1 : 0, rows, &h_));
    }
    template <typename S> std::vector<S> Push(const S *in, size_t n, size_t in_stride = 0, std::vector<float> *track = nullptr) {
        of_kind(sizeof(S));
        return push_tracked<hzsdr_agc_push, S>(in, n, in_stride, track);
    }
    // the rows levelled where they lie (pitch: samples from one row's start to the next; n when 0)
    template <typename S> void PushInPlace(S *rows, size_t n, size_t pitch = 0) {
        of_kind(sizeof(S));
        push_in_place<hzsdr_agc_push>(rows, n, pitch);
    }
    // the same form; the gains and the position stay
    void SetParams(const std::vector<float> &params) { check(x_.raw(), hzsdr_agc_set_params(h_, params.data())); }

private:
    void of_kind(size_t size) const {
        if (size != (kind_ == HZSDR_FMT_C64 ? 8u : 4u)) throw std::invalid_argument("Agc: samples are not of the bank's kind");
    }
    int kind_;
};

// The adaptive equalizer bank (include/hzsdr_equalizer.h): a `taps`-tap linear equalizer at the symbol rate over `rows`
// rows of `kind` (HZSDR_EQUALIZER_REAL_F32: float rows; HZSDR_FMT_C64: std::complex<float> rows), adapted under `mode`
// (HZSDR_EQUALIZER_CMA, _DD_BPSK, _DD_QPSK) with the parameters mu, level shared by all rows, or rows of them when
// per_row.  Push runs min(in_counts[r], n) symbols of every row (row r starts r * in_stride symbols into `in`; dense rows
// when in_stride is 0; every row has n when in_counts is null) and returns dense rows of n values of the input's type (S
// is float or std::complex<float>, as the kind says), zero behind a row's count; where `track` is given it takes dense
// rows of n squared clipped errors.  No flush, no position.  The state: per row the taps, then the taps - 1 latest inputs.
class Equalizer {
public:
    Equalizer(const Context &x, int kind, int mode, size_t taps, size_t centre, const std::vector<float> &params, size_t rows = 1, bool per_row = false)
        : x_(x), rows_(rows), kind_(kind), state_words_(rows * (2 * taps - 1) * (kind == HZSDR_FMT_C64 ? 2 : 1)) {
        if (params.size() != 2 * (per_row ? rows : 1)) throw std::invalid_argument("Equalizer: params are 2, or rows * 2 values");
        check(x_.raw(), hzsdr_equalizer_create(x_.raw(), kind, mode, taps, centre, params.data(), per_row ? 1 : 0, rows, &h_));
    }
    ~Equalizer() { if (h_) hzsdr_equalizer_free(h_); }
    Equalizer(const Equalizer &) = delete;
    Equalizer &operator=(const Equalizer &) = delete;
    template <typename S>
    std::vector<S> Push(const S *in, size_t n, size_t in_stride = 0, const uint32_t *in_counts = nullptr, std::vector<float> *track = nullptr) {
        of_kind(sizeof(S));
        std::vector<S> out(rows_ * n);
        if (track) track->assign(rows_ * n, 0.0f);
        check(x_.raw(), hzsdr_equalizer_push(h_, n ? in : nullptr, n, in_stride ? in_stride : n, in_counts, n ? out.data() : nullptr, n,
                                             track && n ? track->data() : nullptr, n));
        return out;
    }
    // the rows equalized where they lie (pitch: symbols from one row's start to the next; n when 0)
    template <typename S> void PushInPlace(S *rows, size_t n, size_t pitch = 0, const uint32_t *in_counts = nullptr) {
        of_kind(sizeof(S));
        check(x_.raw(), hzsdr_equalizer_push(h_, n ? rows : nullptr, n, pitch ? pitch : n, in_counts, n ? rows : nullptr, pitch ? pitch : n, nullptr, 0));
    }
    // the same form; the state stays
    void SetParams(const std::vector<float> &params) { check(x_.raw(), hzsdr_equalizer_set_params(h_, params.data())); }
    std::vector<float> State() const {
        std::vector<float> z(state_words_);
        check(x_.raw(), hzsdr_equalizer_get_state(h_, z.data(), z.size()));
        return z;
    }
    void SetState(const std::vector<float> &z) { check(x_.raw(), hzsdr_equalizer_set_state(h_, z.data(), z.size())); }
    std::tuple<size_t, size_t, int> Plan() const {
        size_t g = 0, t = 0;
        int f = 0;
        check(x_.raw(), hzsdr_equalizer_plan(h_, &g, &t, &f));
        return {g, t, f};
    }
    void Reset() { check(x_.raw(), hzsdr_equalizer_reset(h_)); }
    size_t Rows() const { return rows_; }

private:
    void of_kind(size_t size) const {
        if (size != (kind_ == HZSDR_FMT_C64 ? 8u : 4u)) throw std::invalid_argument("Equalizer: symbols are not of the bank's kind");
    }
    const Context &x_;
    size_t rows_;
    int kind_;
    size_t state_words_;
    hzsdr_equalizer *h_ = nullptr;
};

// The frame sync bank (include/hzsdr_framesync.h): hard decisions, a search for a sync word of `word_bits` bits under the
// hypotheses (words[h], maps[h]) and the `payload_bits` bits behind every accepted hit, over `rows` rows of soft symbols
// of `kind` (HZSDR_SYMSYNC_REAL_F32: float rows; HZSDR_FMT_C64: std::complex<float> rows, 1 or 2 bits per symbol).  Push
// runs min(in_counts[r], n) symbols of every row (row r starts r * in_stride symbols into `in`; dense rows when in_stride
// is 0; every row has n when in_counts is null) and returns, per row, the frames the push completed, up to `cap` of them;
// a row that accepted more than `cap` throws, since a loss must not pass in silence.  Nothing to flush.
class FrameSync {
public:
    struct Frame {
        std::vector<uint8_t> bytes;  // payload bit k in byte k / 8, bit 7 - k % 8
        uint64_t position;           // the payload's first symbol
        unsigned distance, hypothesis;
    };
    struct Config {
        unsigned bits_per_symbol = 1, word_bits = 0;
        uint64_t mask = 0;  // 0: all word_bits bits
        unsigned thr = 0;
        std::vector<uint64_t> words;
        std::vector<unsigned> maps;
        unsigned payload_bits = 0;
        int diff = 0;
        uint64_t holdoff = 0;  // 0: one frame's symbols
    };
    FrameSync(const Context &x, int kind, const Config &c, size_t rows = 1) : x_(x), rows_(rows), c_(c) {
        if (c.words.empty() || c.words.size() != c.maps.size()) throw std::invalid_argument("FrameSync: a map for every word, at least one");
        const uint64_t mask = c.mask ? c.mask : (c.word_bits >= 64 ? ~0ull : (1ull << c.word_bits) - 1);
        const uint64_t holdoff = c.holdoff ? c.holdoff : (c.word_bits + c.payload_bits) / (c.bits_per_symbol ? c.bits_per_symbol : 1);
        check(x_.raw(), hzsdr_framesync_create(x_.raw(), kind, c.bits_per_symbol, c.word_bits, mask, c.thr, (unsigned)c.words.size(), c.words.data(),
                                               c.maps.data(), c.payload_bits, c.diff, holdoff, rows, &f_));
    }
    ~FrameSync() { if (f_) hzsdr_framesync_free(f_); }
    FrameSync(const FrameSync &) = delete;
    FrameSync &operator=(const FrameSync &) = delete;
    std::vector<std::vector<Frame>> Push(const void *in, size_t n, size_t in_stride = 0, const uint32_t *in_counts = nullptr, size_t cap = 4) {
        const size_t fb = FrameBytes();
        std::vector<uint8_t> out(rows_ * cap * fb);
        std::vector<uint64_t> pos(rows_ * cap);
        std::vector<uint32_t> info(rows_ * cap), counts(rows_, 0);
        size_t most = 0;
        check(x_.raw(), hzsdr_framesync_push(f_, n ? in : nullptr, n, in_stride ? in_stride : n, in_counts, out.data(), cap, cap * fb, pos.data(),
                                             info.data(), counts.data(), &most));
        if (most > cap) throw std::length_error("FrameSync: a row accepted more frames than cap");
        std::vector<std::vector<Frame>> rows(rows_);
        for (size_t r = 0; r < rows_; r++)
            for (size_t f = 0; f < counts[r]; f++) {
                const uint8_t *p = out.data() + (r * cap + f) * fb;
                rows[r].push_back({std::vector<uint8_t>(p, p + fb), pos[r * cap + f], info[r * cap + f] & 0xffu, info[r * cap + f] >> 8});
            }
        return rows;
    }
    struct StateArrays {
        std::vector<uint64_t> positions, holds;
        std::vector<uint8_t> history, last;  // history: rows * ceil(K / 8) bytes, oldest bit first, most significant bit first
    };
    StateArrays State() const {
        StateArrays z{std::vector<uint64_t>(rows_), std::vector<uint64_t>(rows_), std::vector<uint8_t>(rows_ * HistoryBytes()), std::vector<uint8_t>(rows_)};
        check(x_.raw(), hzsdr_framesync_get_state(f_, z.positions.data(), z.holds.data(), z.history.data(), z.last.data(), rows_));
        return z;
    }
    void SetState(const StateArrays &z) {
        if (z.positions.size() != rows_ || z.holds.size() != rows_ || z.history.size() != rows_ * HistoryBytes() || z.last.size() != rows_)
            throw std::invalid_argument("FrameSync: the state has an entry per row");
        check(x_.raw(), hzsdr_framesync_set_state(f_, z.positions.data(), z.holds.data(), z.history.data(), z.last.data(), rows_));
    }
    std::vector<uint64_t> Positions() const {
        std::vector<uint64_t> p(rows_);
        check(x_.raw(), hzsdr_framesync_positions(f_, p.data(), p.size()));
        return p;
    }
    // -> (rows per wave, bits per tile, words of the history ring, HZSDR_FRAMESYNC_FORM_*)
    std::tuple<size_t, size_t, size_t, int> Plan() const {
        size_t g = 0, t = 0, r = 0;
        int f = 0;
        check(x_.raw(), hzsdr_framesync_plan(f_, &g, &t, &r, &f));
        return {g, t, r, f};
    }
    void Reset() { check(x_.raw(), hzsdr_framesync_reset(f_)); }
    size_t Rows() const { return rows_; }
    size_t FrameBytes() const { return (c_.payload_bits + 7) / 8; }
    size_t HistoryBytes() const { return (c_.word_bits + c_.payload_bits - 1 + 7) / 8; }

private:
    const Context &x_;
    size_t rows_;
    Config c_;
    hzsdr_framesync *f_ = nullptr;
};

// The HDLC deframer bank (include/hzsdr_hdlc.h): hard decisions, flags, bit unstuffing and the FCS check over `rows` rows
// of soft symbols of `kind` (HZSDR_SYMSYNC_REAL_F32: float rows; HZSDR_FMT_C64: std::complex<float> rows, Re only).  Push
// takes what FrameSync::Push takes and returns, per row, the frames the push completed, up to `cap` of them, FCS bytes
// included; a row that emitted more than `cap` throws.  Nothing to flush.
class Hdlc {
public:
    struct Frame {
        std::vector<uint8_t> bytes;  // frame bit k in byte k / 8, bit k % 8 (msb_first: bit 7 - k % 8)
        uint64_t position;           // the frame's first bit: the one behind its opening flag
        bool good;                   // the FCS verdict
    };
    struct Config {
        int diff = 0;  // 2: NRZI
        unsigned fcs = 16, min_bytes = 0 /* 0: one more than the FCS */, max_bytes = 256;
        bool msb_first = false, keep_bad = false;
    };
    Hdlc(const Context &x, int kind, const Config &c, size_t rows = 1) : x_(x), rows_(rows), c_(c) {
        if (!c_.min_bytes) c_.min_bytes = c_.fcs / 8 + 1;
        check(x_.raw(), hzsdr_hdlc_create(x_.raw(), kind, c_.diff, c_.fcs, c_.min_bytes, c_.max_bytes, c_.msb_first, c_.keep_bad, rows, &f_));
    }
    ~Hdlc() { if (f_) hzsdr_hdlc_free(f_); }
    Hdlc(const Hdlc &) = delete;
    Hdlc &operator=(const Hdlc &) = delete;
    std::vector<std::vector<Frame>> Push(const void *in, size_t n, size_t in_stride = 0, const uint32_t *in_counts = nullptr, size_t cap = 4) {
        const size_t fb = c_.max_bytes;
        std::vector<uint8_t> out(rows_ * cap * fb);
        std::vector<uint64_t> pos(rows_ * cap);
        std::vector<uint32_t> info(rows_ * cap), counts(rows_, 0);
        size_t most = 0;
        check(x_.raw(), hzsdr_hdlc_push(f_, n ? in : nullptr, n, in_stride ? in_stride : n, in_counts, out.data(), cap, cap * fb, pos.data(), info.data(),
                                        counts.data(), &most));
        if (most > cap) throw std::length_error("Hdlc: a row emitted more frames than cap");
        std::vector<std::vector<Frame>> rows(rows_);
        for (size_t r = 0; r < rows_; r++)
            for (size_t f = 0; f < counts[r]; f++) {
                const uint8_t *p = out.data() + (r * cap + f) * fb;
                const uint32_t i = info[r * cap + f];
                rows[r].push_back({std::vector<uint8_t>(p, p + (i & 0x7fffffffu)), pos[r * cap + f], (i >> 31) != 0});
            }
        return rows;
    }
    struct StateArrays {
        std::vector<uint64_t> positions, events;  // events: the previous event's position plus one
        std::vector<uint8_t> kinds, history, last;  // history: rows * ceil(K / 8) bytes, oldest bit first, most significant bit first
    };
    StateArrays State() const {
        StateArrays z{std::vector<uint64_t>(rows_), std::vector<uint64_t>(rows_), std::vector<uint8_t>(rows_), std::vector<uint8_t>(rows_ * HistoryBytes()),
                      std::vector<uint8_t>(rows_)};
        check(x_.raw(), hzsdr_hdlc_get_state(f_, z.positions.data(), z.events.data(), z.kinds.data(), z.history.data(), z.last.data(), rows_));
        return z;
    }
    void SetState(const StateArrays &z) {
        if (z.positions.size() != rows_ || z.events.size() != rows_ || z.kinds.size() != rows_ || z.history.size() != rows_ * HistoryBytes() ||
            z.last.size() != rows_)
            throw std::invalid_argument("Hdlc: the state has an entry per row");
        check(x_.raw(), hzsdr_hdlc_set_state(f_, z.positions.data(), z.events.data(), z.kinds.data(), z.history.data(), z.last.data(), rows_));
    }
    std::vector<uint64_t> Positions() const {
        std::vector<uint64_t> p(rows_);
        check(x_.raw(), hzsdr_hdlc_positions(f_, p.data(), p.size()));
        return p;
    }
    // -> (rows per wave, bits per tile, words of the history ring, HZSDR_HDLC_FORM_*)
    std::tuple<size_t, size_t, size_t, int> Plan() const {
        size_t g = 0, t = 0, r = 0;
        int f = 0;
        check(x_.raw(), hzsdr_hdlc_plan(f_, &g, &t, &r, &f));
        return {g, t, r, f};
    }
    void Reset() { check(x_.raw(), hzsdr_hdlc_reset(f_)); }
    size_t Rows() const { return rows_; }
    size_t MaxBytes() const { return c_.max_bytes; }
    size_t HistoryBytes() const { return (8 * c_.max_bytes + 8 * c_.max_bytes / 5 + 8 + 7) / 8; }

private:
    const Context &x_;
    size_t rows_;
    Config c_;
    hzsdr_hdlc *f_ = nullptr;
};

// What the three decoder bank classes below share: the handle and its life, the sizes every bank has, the cut of a call's
// results into k = min(in_counts[r], cap) frames per row, and the packing of a list of frames per row into a block of
// slots with counts.  D is the class itself -- its Frame, its frame(bytes, info word) maker and kName, which starts its
// exceptions --, H the handle, Free hzsdr_<bank>_free.
template <class D, class H, auto Free>
class FrameDecoder {
public:
    FrameDecoder(const FrameDecoder &) = delete;
    FrameDecoder &operator=(const FrameDecoder &) = delete;
    size_t Rows() const { return rows_; }
    size_t FrameBytes() const { return fb_; }
    size_t DataBytes() const { return db_; }

protected:
    FrameDecoder(const Context &x, size_t rows) : x_(x), rows_(rows) {}
    ~FrameDecoder() { if (h_) Free(h_); }
    // call(out, info) -> status decodes into dense destinations of `cap` slots a row; the first k frames of every row
    template <class Call> auto decoded(size_t cap, const uint32_t *in_counts, Call call) {
        std::vector<uint8_t> out(rows_ * cap * db_);
        std::vector<uint32_t> info(rows_ * cap);
        check(x_.raw(), call(out.data(), info.data()));
        std::vector<std::vector<typename D::Frame>> rows(rows_);
        for (size_t r = 0; r < rows_; r++) {
            const size_t k = in_counts && in_counts[r] < cap ? in_counts[r] : cap;
            for (size_t f = 0; f < k; f++) {
                const uint8_t *p = out.data() + (r * cap + f) * db_;
                rows[r].push_back(D::frame(std::vector<uint8_t>(p, p + db_), info[r * cap + f]));
            }
        }
        return rows;
    }
    // a list of frames per row (rows_ lists; a frame's bytes are the bank's fb_) as a dense block with counts
    struct Packed {
        size_t cap = 1;
        std::vector<uint8_t> in;
        std::vector<uint32_t> counts;
    };
    template <class In> Packed pack(const std::vector<std::vector<In>> &frames) const {
        Packed p;
        for (const auto &row : frames) p.cap = row.size() > p.cap ? row.size() : p.cap;
        p.in.assign(rows_ * p.cap * fb_, 0);
        p.counts.resize(rows_);
        for (size_t r = 0; r < rows_; r++) {
            p.counts[r] = (uint32_t)frames[r].size();
            for (size_t f = 0; f < frames[r].size(); f++) {
                if (frames[r][f].bytes.size() != fb_) throw std::invalid_argument(std::string(D::kName) + ": a frame of another size");
                std::copy(frames[r][f].bytes.begin(), frames[r][f].bytes.end(), p.in.begin() + (r * p.cap + f) * fb_);
            }
        }
        return p;
    }
    const Context &x_;
    size_t rows_;
    size_t fb_ = 0, db_ = 0;
    H *h_ = nullptr;
};

// The Viterbi decoder bank (include/hzsdr_viterbi.h): frames of a rate 1 / gens.size() convolutional code -- packed hard
// bits (HZSDR_VITERBI_BITS: the frame sync bank's frames as they are) or soft floats (HZSDR_VITERBI_SOFT_F32) -- to
// data_bits data bits, a path metric and a CRC verdict per frame, over `rows` rows of `cap` frame slots.  Decode runs
// min(in_counts[r], cap) frames of every row (row r starts r * in_stride bytes or floats into `in`; dense rows when
// in_stride is 0; every row has cap frames when in_counts is null).  The bank keeps no state.
class Viterbi : public FrameDecoder<Viterbi, hzsdr_viterbi, hzsdr_viterbi_free> {
public:
    static constexpr const char *kName = "Viterbi";
    struct Frame {
        std::vector<uint8_t> bytes;  // data bit k in byte k / 8, bit 7 - k % 8
        uint32_t metric;             // hard input: the channel bit errors corrected
        bool crc_ok;
    };
    static Frame frame(std::vector<uint8_t> bytes, uint32_t w) { return {std::move(bytes), w & 0x7fffffffu, (w >> 31) != 0}; }
    struct Config {
        unsigned K = 7;
        std::vector<unsigned> gens = {0171, 0133};
        unsigned inv = 0;
        uint64_t pattern = 0;  // pattern_bits 0: no puncturing
        unsigned pattern_bits = 0;
        int termination = HZSDR_VITERBI_TAIL;
        size_t data_bits = 0;
        float scale = 1.0f;
        unsigned crc_bits = 0;
        uint32_t crc_poly = 0, crc_init = 0, crc_xorout = 0;
    };
    Viterbi(const Context &x, int kind, const Config &c, size_t rows = 1) : FrameDecoder(x, rows), kind_(kind) {
        if (c.gens.empty()) throw std::invalid_argument("Viterbi: at least two generators");
        const unsigned n = (unsigned)c.gens.size();
        const uint64_t pattern = c.pattern_bits ? c.pattern : (1ull << n) - 1;
        check(x_.raw(), hzsdr_viterbi_create(x_.raw(), kind, c.K, n, c.gens.data(), c.inv, pattern, c.pattern_bits ? c.pattern_bits : n, c.termination,
                                             c.data_bits, c.scale, c.crc_bits, c.crc_poly, c.crc_init, c.crc_xorout, rows, &h_));
        check(x_.raw(), hzsdr_viterbi_sizes(h_, &n_, &fb_, &t_, &db_));
    }
    std::vector<std::vector<Frame>> Decode(const void *in, size_t cap, size_t in_stride = 0, const uint32_t *in_counts = nullptr) {
        const size_t width = cap * (kind_ == HZSDR_VITERBI_BITS ? fb_ : n_);
        return decoded(cap, in_counts, [&](uint8_t *out, uint32_t *info) {
            return hzsdr_viterbi_decode(h_, in, in_stride ? in_stride : width, in_counts, cap, out, cap * db_, info);
        });
    }
    // what FrameSync::Push returned, frame for frame (HZSDR_VITERBI_BITS; a frame's bytes are the bank's FB)
    std::vector<std::vector<Frame>> Decode(const std::vector<std::vector<FrameSync::Frame>> &frames) {
        if (kind_ != HZSDR_VITERBI_BITS || frames.size() != rows_) throw std::invalid_argument("Viterbi: hard-bit frames, a list per row");
        const Packed p = pack(frames);
        return Decode(p.in.data(), p.cap, 0, p.counts.data());
    }
    // -> (frames per wave, states per lane, bytes of a frame's decisions, HZSDR_VITERBI_FORM_*)
    std::tuple<size_t, size_t, size_t, int> Plan() const {
        size_t g = 0, s = 0, d = 0;
        int f = 0;
        check(x_.raw(), hzsdr_viterbi_plan(h_, &g, &s, &d, &f));
        return {g, s, d, f};
    }
    size_t ReceivedBits() const { return n_; }
    size_t Steps() const { return t_; }

private:
    int kind_;
    size_t n_ = 0, t_ = 0;
};

// The LDPC decoder bank (include/hzsdr_ldpc.h): frames of a binary LDPC code given by its parity-check matrix in
// check-major compressed form -- soft floats (HZSDR_LDPC_SOFT_F32: the soft frame bank's values as they are) or packed
// hard bits (HZSDR_LDPC_BITS: the frame sync bank's frames) -- decoded by flooding min-sum in integers to data_bits data
// bits, the unsatisfied checks, the iterations run and a verdict per frame, over `rows` rows of `cap` frame slots.
// Decode runs min(in_counts[r], cap) frames of every row (row r starts r * in_stride bytes or floats into `in`; dense
// rows when in_stride is 0; every row has cap frames when in_counts is null).  The bank keeps no state.
class Ldpc : public FrameDecoder<Ldpc, hzsdr_ldpc, hzsdr_ldpc_free> {
public:
    static constexpr const char *kName = "Ldpc";
    struct Frame {
        std::vector<uint8_t> bytes;  // data bit k in byte k / 8, bit 7 - k % 8
        uint32_t unsatisfied;        // checks of odd parity behind the last iteration run
        uint32_t iters;              // iterations run
        bool ok;                     // unsatisfied == 0
    };
    static Frame frame(std::vector<uint8_t> bytes, uint32_t w) { return {std::move(bytes), w & 0xffffu, (w >> 16) & 0xffu, (w >> 31) != 0}; }
    struct Config {
        size_t variables = 0;
        std::vector<uint32_t> row_ptr, col;  // checks + 1 entries; the variables of every check, ascending
        size_t head = 0;
        size_t received = 0;   // 0: every variable behind head
        size_t data_bits = 0;  // 0: every variable
        float scale = 1.0f;
        unsigned level = 1, max_iters = 50, norm = 12, offset = 0;
    };
    Ldpc(const Context &x, int kind, const Config &c, size_t rows = 1) : FrameDecoder(x, rows), kind_(kind) {
        if (c.row_ptr.empty() || c.head > c.variables) throw std::invalid_argument("Ldpc: row_ptr has checks + 1 entries, head is at most variables");
        check(x_.raw(), hzsdr_ldpc_create(x_.raw(), kind, c.row_ptr.size() - 1, c.variables, c.row_ptr.data(), c.col.data(), c.col.size(), c.head,
                                          c.received ? c.received : c.variables - c.head, c.data_bits ? c.data_bits : c.variables, c.scale, c.level,
                                          c.max_iters, c.norm, c.offset, rows, &h_));
        check(x_.raw(), hzsdr_ldpc_sizes(h_, &n_, &fb_, &vars_, &checks_, &edges_, &db_));
    }
    std::vector<std::vector<Frame>> Decode(const void *in, size_t cap, size_t in_stride = 0, const uint32_t *in_counts = nullptr) {
        const size_t width = cap * (kind_ == HZSDR_LDPC_BITS ? fb_ : n_);
        return decoded(cap, in_counts, [&](uint8_t *out, uint32_t *info) {
            return hzsdr_ldpc_decode(h_, in, in_stride ? in_stride : width, in_counts, cap, out, cap * db_, info);
        });
    }
    // what FrameSync::Push returned, frame for frame (HZSDR_LDPC_BITS; a frame's bytes are the bank's FB)
    std::vector<std::vector<Frame>> Decode(const std::vector<std::vector<FrameSync::Frame>> &frames) {
        if (kind_ != HZSDR_LDPC_BITS || frames.size() != rows_) throw std::invalid_argument("Ldpc: hard-bit frames, a list per row");
        const Packed p = pack(frames);
        return Decode(p.in.data(), p.cap, 0, p.counts.data());
    }
    // -> (frames per workgroup, threads per frame, LDS bytes of a frame's state, HZSDR_LDPC_FORM_*)
    std::tuple<size_t, size_t, size_t, int> Plan() const {
        size_t g = 0, t = 0, b = 0;
        int f = 0;
        check(x_.raw(), hzsdr_ldpc_plan(h_, &g, &t, &b, &f));
        return {g, t, b, f};
    }
    size_t ReceivedBits() const { return n_; }
    size_t Variables() const { return vars_; }
    size_t Checks() const { return checks_; }
    size_t Edges() const { return edges_; }

private:
    int kind_;
    size_t n_ = 0, vars_ = 0, checks_ = 0, edges_ = 0;
};

// The demapper bank (include/hzsdr_demap.h): frames of received symbols -- complex (HZSDR_DEMAP_C64: the soft frame bank's
// floats re, im ...), real (HZSDR_DEMAP_REAL_F32) or per-bit values already (HZSDR_DEMAP_LLR_F32) -- to max-log soft values
// against 2^m points listed by label, scaled by a gain (one, or one per row), put into the decoder's order by perm
// (HZSDR_DEMAP_ERASED marks a hole) and sign by flip, over `rows` rows of `cap` frame slots: what Viterbi and Ldpc read as
// soft input.  Run handles min(in_counts[r], cap) frames of every row (row r starts r * in_stride floats into `in`; dense
// rows when in_stride is 0; every row has cap frames when in_counts is null).  The bank keeps no state.
class Demapper {
public:
    struct Config {
        unsigned bits_per_symbol = 1;
        std::vector<float> points;  // 2 M floats re, im (C64), M floats (REAL_F32), none (LLR_F32)
        size_t symbols = 0;
        std::vector<uint32_t> perm;  // empty: the order is kept, N = symbols * bits_per_symbol
        std::vector<uint8_t> flip;   // empty: no sign is flipped; else ceil(N / 8) packed bytes
        std::vector<float> gains = {1.0f};
    };
    Demapper(const Context &x, int kind, const Config &c, size_t rows = 1) : x_(x), rows_(rows) {
        const size_t n = c.perm.empty() ? c.symbols * c.bits_per_symbol : c.perm.size();
        if (!c.flip.empty() && c.flip.size() != (n + 7) / 8) throw std::invalid_argument("Demapper: flip has ceil(N / 8) bytes");
        check(x_.raw(), hzsdr_demap_create(x_.raw(), kind, c.bits_per_symbol, c.points.empty() ? nullptr : c.points.data(), c.symbols,
                                           c.perm.empty() ? nullptr : c.perm.data(), n, c.flip.empty() ? nullptr : c.flip.data(),
                                           c.gains.empty() ? nullptr : c.gains.data(), c.gains.size(), rows, &h_));
        check(x_.raw(), hzsdr_demap_sizes(h_, &s_, &w_, &m_, &n_));
    }
    Demapper(const Demapper &) = delete;
    Demapper &operator=(const Demapper &) = delete;
    ~Demapper() { if (h_) hzsdr_demap_free(h_); }
    // into `out`, rows of out_stride floats (dense rows of cap * N when 0)
    void Run(const float *in, size_t cap, float *out, size_t in_stride = 0, const uint32_t *in_counts = nullptr, size_t out_stride = 0) {
        check(x_.raw(), hzsdr_demap_run(h_, in, in_stride ? in_stride : cap * w_, in_counts, cap, out, out_stride ? out_stride : cap * n_));
    }
    // -> a dense block (rows, cap, N); slots behind a row's count are zero
    std::vector<float> Run(const float *in, size_t cap, size_t in_stride = 0, const uint32_t *in_counts = nullptr) {
        std::vector<float> out(rows_ * cap * n_, 0.0f);
        Run(in, cap, out.data(), in_stride, in_counts);
        return out;
    }
    // -> (frames per workgroup, threads per frame, LDS bytes of a frame's values, a sum of HZSDR_DEMAP_FORM_*)
    std::tuple<size_t, size_t, size_t, int> Plan() const {
        size_t g = 0, t = 0, b = 0;
        int f = 0;
        check(x_.raw(), hzsdr_demap_plan(h_, &g, &t, &b, &f));
        return {g, t, b, f};
    }
    size_t Rows() const { return rows_; }
    size_t Symbols() const { return s_; }
    size_t FrameFloats() const { return w_; }
    size_t BitsPerSymbol() const { return m_; }
    size_t Values() const { return n_; }

private:
    const Context &x_;
    size_t rows_;
    size_t s_ = 0, w_ = 0, m_ = 0, n_ = 0;
    hzsdr_demap *h_ = nullptr;
};

// The Reed-Solomon decoder bank (include/hzsdr_rs.h): frames of `interleave` symbol-interleaved codewords over GF(2^8) --
// the Viterbi bank's decoded frames as they are -- to corrected data bytes and a verdict per frame, over `rows` rows of
// `cap` frame slots.  Decode runs min(in_counts[r], cap) frames of every row (row r starts r * in_stride bytes into `in`,
// frame f of it f * in_pitch bytes further; dense rows and slots when they are 0; every row has cap frames when in_counts
// is null).  The bank keeps no state.
class ReedSolomon : public FrameDecoder<ReedSolomon, hzsdr_rs, hzsdr_rs_free> {
public:
    static constexpr const char *kName = "ReedSolomon";
    struct Frame {
        std::vector<uint8_t> bytes;  // the I k data bytes, corrected where the codeword did not fail
        uint32_t errors, failed;     // symbols corrected over the frame's decoded codewords; codewords that failed
        bool ok;                     // failed == 0
    };
    static Frame frame(std::vector<uint8_t> bytes, uint32_t w) { return {std::move(bytes), w & 0xffffu, (w >> 16) & 0x7fffu, (w >> 31) != 0}; }
    struct Config {
        unsigned gfpoly = 0x187, fcr = 112, prim = 11, nroots = 32, n = 255;  // CCSDS 255/223
        unsigned interleave = 1;
        std::vector<uint8_t> in_map, out_map;  // empty: identity; else 256 bytes
        std::vector<uint8_t> scramble;         // empty: none
    };
    ReedSolomon(const Context &x, const Config &c, size_t rows = 1) : FrameDecoder(x, rows) {
        if ((!c.in_map.empty() && c.in_map.size() != 256) || (!c.out_map.empty() && c.out_map.size() != 256))
            throw std::invalid_argument("ReedSolomon: a map is 256 bytes");
        check(x_.raw(), hzsdr_rs_create(x_.raw(), c.gfpoly, c.fcr, c.prim, c.nroots, c.n, c.interleave, c.in_map.empty() ? nullptr : c.in_map.data(),
                                        c.out_map.empty() ? nullptr : c.out_map.data(), c.scramble.empty() ? nullptr : c.scramble.data(), c.scramble.size(),
                                        rows, &h_));
        check(x_.raw(), hzsdr_rs_sizes(h_, &k_, &t_, &fb_, &db_));
    }
    std::vector<std::vector<Frame>> Decode(const uint8_t *in, size_t cap, size_t in_stride = 0, size_t in_pitch = 0, const uint32_t *in_counts = nullptr) {
        const size_t pitch = in_pitch ? in_pitch : fb_;
        return decoded(cap, in_counts, [&](uint8_t *out, uint32_t *info) {
            return hzsdr_rs_decode(h_, in, in_stride ? in_stride : cap * pitch, pitch, in_counts, cap, out, cap * db_, db_, info);
        });
    }
    // what Viterbi::Decode returned, frame for frame (a frame's bytes are the bank's frame bytes)
    std::vector<std::vector<Frame>> Decode(const std::vector<std::vector<Viterbi::Frame>> &frames) {
        if (frames.size() != rows_) throw std::invalid_argument("ReedSolomon: a list of frames per row");
        const Packed p = pack(frames);
        return Decode(p.in.data(), p.cap, 0, 0, p.counts.data());
    }
    // -> (waves per workgroup, LDS bytes per workgroup, workgroups a compute unit holds, workgroups of a call at most)
    std::tuple<size_t, size_t, size_t, size_t> Plan() const {
        size_t w = 0, l = 0, c = 0, g = 0;
        check(x_.raw(), hzsdr_rs_plan(h_, &w, &l, &c, &g));
        return {w, l, c, g};
    }
    size_t DataSymbols() const { return k_; }
    size_t Correctable() const { return t_; }

private:
    size_t k_ = 0, t_ = 0;
};

// The tuner bank (include/hzsdr_tuner.h): one pass over a stream of src_format samples, a tuner per frequency word
// (word = round(f / fs * 2^32) mod 2^32), the shared prototype filter `taps` and a decimation by `down`; complex64.
// Push consumes `n` samples and returns the outputs they complete as dense rows, row k of the returned count per row
// at [k * count, (k + 1) * count); Flush returns the outputs that still depend on samples pushed and starts over.
class TunerBank {
public:
    TunerBank(const Context &x, int src_format, const std::vector<uint32_t> &words, const std::vector<float> &taps, size_t down = 1)
        : x_(x), tuners_(words.size()), qp_((taps.size() + 1) & ~(size_t)1) {
        check(x_.raw(), hzsdr_tuner_create(x_.raw(), src_format, words.data(), words.size(), down, taps.data(), taps.size(), &t_));
    }
    ~TunerBank() { if (t_) hzsdr_tuner_free(t_); }
    TunerBank(const TunerBank &) = delete;
    TunerBank &operator=(const TunerBank &) = delete;
    std::vector<std::complex<float>> Push(const void *in, size_t n) {
        const size_t count = OutputsFor(n);
        std::vector<std::complex<float>> out(tuners_ * count);
        size_t w = 0;
        check(x_.raw(), hzsdr_tuner_push(t_, n ? in : nullptr, n, count ? out.data() : nullptr, count, count, &w));
        return out;
    }
    std::vector<std::complex<float>> Flush() {
        const size_t count = std::get<2>(Pending());
        std::vector<std::complex<float>> out(tuners_ * count);
        size_t w = 0;
        check(x_.raw(), hzsdr_tuner_flush(t_, count ? out.data() : nullptr, count, count, &w));
        return out;
    }
    size_t OutputsFor(size_t n) const {
        size_t c = 0;
        check(x_.raw(), hzsdr_tuner_outputs_for(t_, n, &c));
        return c;
    }
    // -> (samples consumed, index of the next output, outputs per row a flush would write now)
    std::tuple<uint64_t, uint64_t, size_t> Pending() const {
        uint64_t n = 0, m = 0;
        size_t f = 0;
        check(x_.raw(), hzsdr_tuner_pending(t_, &n, &m, &f));
        return {n, m, f};
    }
    // -> (outputs per workgroup, rows of the real matrix per workgroup, HZSDR_TUNER_FORM_*)
    std::tuple<size_t, size_t, int> Plan() const {
        size_t t = 0, r = 0;
        int f = 0;
        check(x_.raw(), hzsdr_tuner_plan(t_, &t, &r, &f));
        return {t, r, f};
    }
    // the words of tuners [first, first + words.size()), in effect from the next push on
    void Retune(size_t first, const std::vector<uint32_t> &words) { check(x_.raw(), hzsdr_tuner_set_words(t_, first, words.size(), words.data())); }
    // HZSDR_TUNER_READ_TAPS of tuner `index` (the taps rounded up to an even count of complex64 values), or one of the three tables
    std::vector<std::complex<float>> Readout(int what, size_t index = 0) const {
        std::vector<std::complex<float>> out(what == HZSDR_TUNER_READ_TAPS ? qp_ : what == HZSDR_TUNER_READ_T0 ? 1024 : 2048);
        check(x_.raw(), hzsdr_tuner_readout(t_, what, index, out.data(), out.size()));
        return out;
    }
    void Reset() { check(x_.raw(), hzsdr_tuner_reset(t_)); }
    size_t Tuners() const { return tuners_; }

private:
    const Context &x_;
    size_t tuners_, qp_;
    hzsdr_tuner *t_ = nullptr;
};

// The soft frame bank (include/hzsdr_softframe.h) beside a FrameSync of the same kind, configuration and rows: Push takes
// the symbols that FrameSync::Push got and the frames it returned and gives, frame for frame, the payload's floats through
// the frame's hypothesis map -- what a Viterbi of HZSDR_VITERBI_SOFT_F32 input reads -- and a status
// (HZSDR_SOFTFRAME_SERVED for every frame the FrameSync emitted in the same push).  A FrameSync configuration with a
// differential decoding has no soft counterpart and is refused.
class SoftFrames {
public:
    struct Frame {
        std::vector<float> values;  // float k decides payload bit k: sign bit clear means 1
        uint32_t status;
    };
    SoftFrames(const Context &x, int kind, const FrameSync::Config &c, size_t rows = 1) : x_(x), rows_(rows), p_(c.payload_bits) {
        if (c.diff != 0) throw std::invalid_argument("SoftFrames: a differential decoding has no soft counterpart");
        if (c.maps.empty()) throw std::invalid_argument("SoftFrames: at least one map");
        check(x_.raw(), hzsdr_softframe_create(x_.raw(), kind, c.bits_per_symbol, c.payload_bits, (unsigned)c.maps.size(), c.maps.data(), rows, &f_));
    }
    ~SoftFrames() { if (f_) hzsdr_softframe_free(f_); }
    SoftFrames(const SoftFrames &) = delete;
    SoftFrames &operator=(const SoftFrames &) = delete;
    // the arrays of hzsdr_framesync_push as they are
    void Push(const void *in, size_t n, size_t in_stride, const uint32_t *in_counts, const uint64_t *positions, const uint32_t *info,
              const uint32_t *counts, size_t cap, float *out, size_t out_stride, uint32_t *status) {
        check(x_.raw(), hzsdr_softframe_push(f_, n ? in : nullptr, n, in_stride ? in_stride : n, in_counts, positions, info, counts, cap, out, out_stride, status));
    }
    // what FrameSync::Push(in, n, in_stride, in_counts, ...) returned, frame for frame
    std::vector<std::vector<Frame>> Push(const void *in, size_t n, const std::vector<std::vector<FrameSync::Frame>> &frames, size_t in_stride = 0,
                                         const uint32_t *in_counts = nullptr) {
        if (frames.size() != rows_) throw std::invalid_argument("SoftFrames: a list of frames per row");
        size_t cap = 0;
        for (const auto &row : frames) cap = row.size() > cap ? row.size() : cap;
        std::vector<uint64_t> pos(rows_ * cap);
        std::vector<uint32_t> info(rows_ * cap), counts(rows_), status(rows_ * cap);
        std::vector<float> out(rows_ * cap * p_);
        for (size_t r = 0; r < rows_; r++) {
            counts[r] = (uint32_t)frames[r].size();
            for (size_t f = 0; f < frames[r].size(); f++) {
                pos[r * cap + f] = frames[r][f].position;
                info[r * cap + f] = frames[r][f].distance | frames[r][f].hypothesis << 8;
            }
        }
        Push(in, n, in_stride, in_counts, pos.data(), info.data(), counts.data(), cap, out.data(), cap * p_, status.data());
        std::vector<std::vector<Frame>> rows(rows_);
        for (size_t r = 0; r < rows_; r++)
            for (size_t f = 0; f < frames[r].size(); f++) {
                const float *p = out.data() + (r * cap + f) * p_;
                rows[r].push_back({std::vector<float>(p, p + p_), status[r * cap + f]});
            }
        return rows;
    }
    struct StateArrays {
        std::vector<uint64_t> positions;
        std::vector<float> history;  // rows * HistoryFloats(), oldest first
    };
    StateArrays State() const {
        StateArrays z{std::vector<uint64_t>(rows_), std::vector<float>(rows_ * HistoryFloats())};
        check(x_.raw(), hzsdr_softframe_get_state(f_, z.positions.data(), z.history.empty() ? nullptr : z.history.data(), rows_));
        return z;
    }
    void SetState(const StateArrays &z) {
        if (z.positions.size() != rows_ || z.history.size() != rows_ * HistoryFloats()) throw std::invalid_argument("SoftFrames: the state has an entry per row");
        check(x_.raw(), hzsdr_softframe_set_state(f_, z.positions.data(), z.history.empty() ? nullptr : z.history.data(), rows_));
    }
    std::vector<uint64_t> Positions() const {
        std::vector<uint64_t> p(rows_);
        check(x_.raw(), hzsdr_softframe_positions(f_, p.data(), p.size()));
        return p;
    }
    // -> (floats a workgroup moves per step, history floats per row, HZSDR_SOFTFRAME_FORM_*)
    std::tuple<size_t, size_t, int> Plan() const {
        size_t s = 0, h = 0;
        int f = 0;
        check(x_.raw(), hzsdr_softframe_plan(f_, &s, &h, &f));
        return {s, h, f};
    }
    void Reset() { check(x_.raw(), hzsdr_softframe_reset(f_)); }
    size_t Rows() const { return rows_; }
    size_t PayloadBits() const { return p_; }
    size_t HistoryFloats() const { return std::get<1>(Plan()); }

private:
    const Context &x_;
    size_t rows_, p_;
    hzsdr_softframe *f_ = nullptr;
};
}  // namespace stream

namespace array {

// The covariance bank (include/hzsdr_covar.h): `channels` coherent rows (2 ... 16) of one format into their spatial
// covariance, one unnormalised channels x channels complex64 matrix, row-major, per `block` snapshots.  Push consumes
// every snapshot it is given -- one buffer per channel, as Context::Beamform takes them -- and returns the matrices of
// the blocks that complete, one behind the other; Flush returns the open block's (or nothing) and starts over.
class Covariance {
public:
    Covariance(const Context &x, int src_format, size_t channels, size_t block) : x_(x), n_(channels), b_(block) {
        check(x_.raw(), hzsdr_covar_create(x_.raw(), src_format, channels, block, &c_));
    }
    ~Covariance() { if (c_) hzsdr_covar_free(c_); }
    Covariance(const Covariance &) = delete;
    Covariance &operator=(const Covariance &) = delete;
    size_t BlocksFor(size_t n_in) const {
        size_t b = 0;
        check(x_.raw(), hzsdr_covar_blocks_for(c_, n_in, &b));
        return b;
    }
    // (a HOST context's buffers: the matrices come back in a vector)
    std::vector<std::complex<float>> Push(const std::vector<Samples> &channels) {
        if (channels.size() != n_) throw Error(HZSDR_ERR_INVALID_ARGUMENT, "covariance: one buffer per channel");
        std::vector<const void *> rows;
        for (const Samples &s : channels) {
            if (s.length != channels[0].length) throw Error(HZSDR_ERR_LENGTH_MISMATCH, "covariance: the channels' buffers have one length");
            rows.push_back(s.data);
        }
        const size_t want = BlocksFor(channels[0].length);
        std::vector<std::complex<float>> out(want * n_ * n_);
        size_t got = 0;
        check(x_.raw(), hzsdr_covar_push_channels(c_, rows.data(), channels[0].length, out.empty() ? nullptr : out.data(), want, n_ * n_, &got));
        return out;
    }
    // one channel-major block: row i starts i * stride samples into `in`, `n` snapshots per row
    std::vector<std::complex<float>> PushRows(const void *in, size_t n, size_t stride) {
        const size_t want = BlocksFor(n);
        std::vector<std::complex<float>> out(want * n_ * n_);
        size_t got = 0;
        check(x_.raw(), hzsdr_covar_push(c_, in, n, stride, out.empty() ? nullptr : out.data(), want, n_ * n_, &got));
        return out;
    }
    std::vector<std::complex<float>> Flush() {
        std::vector<std::complex<float>> out(n_ * n_);
        size_t got = 0;
        check(x_.raw(), hzsdr_covar_flush(c_, out.data(), 1, &got));
        out.resize(got * n_ * n_);
        return out;
    }
    // -> (snapshots consumed per row, index of the open block, snapshots it holds)
    std::tuple<uint64_t, uint64_t, size_t> Pending() const {
        uint64_t c = 0, b = 0;
        size_t o = 0;
        check(x_.raw(), hzsdr_covar_pending(c_, &c, &b, &o));
        return {c, b, o};
    }
    // -> (segment length, segments of a workgroup's group, HZSDR_COVAR_FORM_*)
    std::tuple<size_t, size_t, int> Plan() const {
        size_t s = 0, g = 0;
        int f = 0;
        check(x_.raw(), hzsdr_covar_plan(c_, &s, &g, &f));
        return {s, g, f};
    }
    void Reset() { check(x_.raw(), hzsdr_covar_reset(c_)); }
    size_t Channels() const { return n_; }
    size_t Block() const { return b_; }

private:
    const Context &x_;
    size_t n_, b_;
    hzsdr_covar *c_ = nullptr;
};

// The beam scan (include/hzsdr_covar.h) over `weights`, vectors x channels complex64 as hzsdr_beamform_angles makes
// them: Run maps channels x channels matrices Q, one behind the other, to p[b][g] = Re w_g Q_b w_g^H.
class Scan {
public:
    Scan(const Context &x, size_t channels, const std::vector<std::complex<float>> &weights)
        : x_(x), n_(channels), g_(channels ? weights.size() / channels : 0) {
        if (channels == 0 || weights.size() % channels) throw Error(HZSDR_ERR_INVALID_ARGUMENT, "scan: the weights are vectors x channels");
        check(x_.raw(), hzsdr_scan_create(x_.raw(), channels, weights.data(), g_, &s_));
    }
    ~Scan() { if (s_) hzsdr_scan_free(s_); }
    Scan(const Scan &) = delete;
    Scan &operator=(const Scan &) = delete;
    std::vector<float> Run(const std::vector<std::complex<float>> &mats) {
        const size_t count = mats.size() / (n_ * n_);
        if (mats.size() != count * n_ * n_) throw Error(HZSDR_ERR_LENGTH_MISMATCH, "scan: matrices are channels x channels");
        std::vector<float> out(count * g_);
        check(x_.raw(), hzsdr_scan_run(s_, mats.data(), count, n_ * n_, out.data(), out.size(), g_));
        return out;
    }
    size_t Vectors() const { return g_; }

private:
    const Context &x_;
    size_t n_, g_;
    hzsdr_scan *s_ = nullptr;
};

}  // namespace array
}  // namespace hzsdr
