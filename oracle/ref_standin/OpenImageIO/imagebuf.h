// Stand-in for <OpenImageIO/imagebuf.h>, written for this project (see ../README.md): data carriers only.
// ImageInput::open serves float images the driver registered under a name, so that MeshEngine::bindTexture
// runs as written; ImageBuf::write encodes nothing and hands the buffer to a hook the driver may install,
// so that Camera::saveFrame's conversion can be read back without a file being written.
#pragma once
#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace OpenImageIO {

struct TypeDesc {
    enum BASETYPE { UNKNOWN, UINT8, FLOAT };
    BASETYPE basetype;
    TypeDesc(BASETYPE b = UNKNOWN) : basetype(b) {}
};

struct ImageSpec {
    int width, height, nchannels;
    TypeDesc format;
    ImageSpec(int w = 0, int h = 0, int c = 0, TypeDesc f = TypeDesc::UINT8) : width(w), height(h), nchannels(c), format(f) {}
};

struct standin_image {
    ImageSpec spec;
    std::vector<float> pixels;  // row-major, channels interleaved: the order read_image delivers
};
inline std::map<std::string, standin_image> &standin_images() {
    static std::map<std::string, standin_image> images;
    return images;
}
inline void standin_register_image(const std::string &name, int w, int h, int c, const float *data) {
    standin_image &im = standin_images()[name];
    im.spec = ImageSpec(w, h, c, TypeDesc::FLOAT);
    im.pixels.assign(data, data + (std::size_t)w * h * c);
}

class ImageInput {
    const standin_image *im;
    explicit ImageInput(const standin_image *i) : im(i) {}

   public:
    static ImageInput *open(const std::string &name) {
        auto it = standin_images().find(name);
        return it == standin_images().end() ? nullptr : new ImageInput(&it->second);
    }
    const ImageSpec &spec() const { return im->spec; }
    bool read_image(TypeDesc, void *data) {
        std::memcpy(data, im->pixels.data(), im->pixels.size() * sizeof(float));
        return true;
    }
    bool close() { return true; }
    static void destroy(ImageInput *in) { delete in; }
};

typedef void (*standin_write_hook)(const std::string &name, const ImageSpec &spec, const void *pixels);
inline standin_write_hook &standin_on_write() {
    static standin_write_hook hook = nullptr;
    return hook;
}

class ImageBuf {
    ImageSpec spec_;
    const void *pixels_;

   public:
    ImageBuf(const ImageSpec &spec, void *pixels) : spec_(spec), pixels_(pixels) {}
    bool write(const std::string &name, const std::string & = std::string()) const {
        if (standin_on_write()) standin_on_write()(name, spec_, pixels_);
        return true;
    }
};

}  // namespace OpenImageIO
namespace OIIO = OpenImageIO;
