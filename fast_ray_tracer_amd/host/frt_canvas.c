/*
 * frt-mi355x host: canvas storage and image I/O.
 *
 * The output contract of the drop-in boundary is the reference's: a Color
 * (double[4]) canvas, row 0 at the top, written as a 16-bit big-endian P6 PPM
 * with the reference's normalisation (reference src/libs/canvas/canvas.c:150-327)
 * and as a 16-bit sRGB PNG through libpng (canvas.c:376-510). Texture readers
 * (PNG, ASCII PPM) follow canvas.c:330-672. The 16-bit values come from the host
 * pass below or, byte-identical, from the device (FRT_ENCODE, frt_encode.hip); the
 * file and libpng writing stay here.
 */
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <png.h>

#include "src/libs/canvas/canvas.h"
#include "src/color/rgb.h"
#include "src/libs/linalg/linalg.h"
#include "frt_device.h"

#define FRT_SQRT3 1.7320508075688772

/*
 * A canvas with a word of our own behind the reference's struct: the byte size of its array when that array is
 * page-locked (frt_canvas_alloc_pinned), 0 when malloc'd. render_multi's canvas is page-locked so that the device's
 * copy of the frame is one DMA into it (into malloc'd memory the runtime stages it through its own buffers, and a
 * fresh 66 MB array at 1920x1080 first takes ~16 000 page faults); canvas_free hands such an array to a one-entry
 * pool that the next render_multi of the same size takes again. Page-locked memory is a scarce kind: at most
 * FRT_PINNED_CANVASES (default 4) such arrays are out in live canvases at once, and a canvas asked for beyond that
 * (a camera loop that keeps every frame) gets an ordinary malloc'd array, as canvas_alloc gives.
 */
typedef struct {
    struct canvas c;
    size_t pinned_bytes;
} canvas_box;

static pthread_mutex_t g_pool_lock = PTHREAD_MUTEX_INITIALIZER;
static void *g_pool_arr;     /* an idle page-locked array */
static size_t g_pool_bytes;
static size_t g_pinned_out;  /* page-locked arrays held by live canvases */

static size_t
pinned_cap(void)
{
    const char *e = getenv("FRT_PINNED_CANVASES");
    return e != NULL && *e ? (size_t)strtoul(e, NULL, 10) : 4;
}

static Canvas
canvas_new(size_t width, size_t height, bool super_sample, void (*color_space_fn)(const Color, Color))
{
    canvas_box *b = (canvas_box *)malloc(sizeof(canvas_box));
    if (b == NULL) {
        return NULL;
    }
    b->pinned_bytes = 0;
    b->c.arr = NULL;
    b->c.width = width;
    b->c.height = height;
    b->c.super_sample = super_sample;
    b->c.color_space_fn = color_space_fn;
    return &b->c;
}

Canvas
canvas_alloc(size_t width, size_t height, bool super_sample, void (*color_space_fn)(const Color, Color))
{
    Canvas c = canvas_new(width, height, super_sample, color_space_fn);
    if (c != NULL) {
        c->arr = (Color *)malloc(width * height * sizeof(Color));
    }
    return c;
}

Canvas
frt_canvas_alloc_pinned(size_t width, size_t height, bool super_sample, void (*color_space_fn)(const Color, Color))
{
    Canvas c = canvas_new(width, height, super_sample, color_space_fn);
    if (c == NULL) {
        return NULL;
    }
    const size_t bytes = width * height * sizeof(Color);
    void *stale = NULL;
    const size_t cap = pinned_cap();
    pthread_mutex_lock(&g_pool_lock);
    const int over = g_pinned_out >= cap;
    if (over) {
        /* (the pool's idle array stays for the next canvas under the cap) */
    } else if (g_pool_arr != NULL && g_pool_bytes == bytes) {
        c->arr = (Color *)g_pool_arr;
        g_pool_arr = NULL;
    } else {
        stale = g_pool_arr;  /* (another size: freed, outside the lock) */
        g_pool_arr = NULL;
    }
    pthread_mutex_unlock(&g_pool_lock);
    frt_host_pinned_free(stale);
    if (c->arr == NULL && !over) {
        c->arr = (Color *)frt_host_pinned_alloc(bytes);
    }
    if (c->arr != NULL) {
        ((canvas_box *)c)->pinned_bytes = bytes;
        pthread_mutex_lock(&g_pool_lock);
        ++g_pinned_out;
        pthread_mutex_unlock(&g_pool_lock);
    } else {
        c->arr = (Color *)malloc(bytes);  /* (no page-locked memory: an ordinary array) */
    }
    return c;
}

/* diagnostics: 1 when the canvas's array is page-locked (counts towards FRT_PINNED_CANVASES), 0 when malloc'd */
int
frt_canvas_is_pinned(Canvas c)
{
    return c != NULL && ((canvas_box *)c)->pinned_bytes > 0;
}

void
frt_canvas_pool_release(void)
{
    pthread_mutex_lock(&g_pool_lock);
    void *p = g_pool_arr;
    g_pool_arr = NULL;
    g_pool_bytes = 0;
    pthread_mutex_unlock(&g_pool_lock);
    frt_host_pinned_free(p);
}

Ppm
ppm_alloc(size_t len)
{
    Ppm p = (Ppm)malloc(sizeof(struct ppm_struct));
    p->arr = (unsigned char *)malloc(len);
    p->len = len;
    return p;
}

void
canvas_free(Canvas c)
{
    if (c == NULL) {
        return;
    }
    canvas_box *b = (canvas_box *)c;
    if (b->pinned_bytes > 0) {
        void *spill = c->arr;
        pthread_mutex_lock(&g_pool_lock);
        --g_pinned_out;
        if (g_pool_arr == NULL) {
            g_pool_arr = c->arr;
            g_pool_bytes = b->pinned_bytes;
            spill = NULL;
        }
        pthread_mutex_unlock(&g_pool_lock);
        frt_host_pinned_free(spill);
    } else {
        free(c->arr);
    }
    free(b);
}

void
ppm_free(Ppm p)
{
    if (p) {
        free(p->arr);
        free(p);
    }
}

void
canvas_write_pixels(Canvas c, int col, int row, Color *colors, size_t num)
{
    memcpy(c->arr + (size_t)row * c->width + col, colors, num * sizeof(Color));
}

void
canvas_write_pixel(Canvas c, int col, int row, Color color)
{
    memcpy(c->arr[(size_t)row * c->width + col], color, sizeof(Color));
}

void
canvas_pixel_at(Canvas c, int col, int row, Color res)
{
    /* reference canvas.c:115-148: optional 3x3 wrap-around box filter, then
     * the canvas's color-space function per fetch */
    if (!c->super_sample) {
        c->color_space_fn(c->arr[(size_t)row * c->width + col], res);
        return;
    }
    Color acc = {0.0, 0.0, 0.0, 0.0};
    int w = (int)c->width, h = (int)c->height;
    int cc = col - 1;
    for (int j = 0; j < 3; ++j, ++cc) {
        if (cc < 0) cc += w;
        if (cc == w) cc = 0;
        int rr = row - 1;
        for (int i = 0; i < 3; ++i, ++rr) {
            if (rr < 0) rr += h;
            if (rr == h) rr = 0;
            color_accumulate(acc, c->arr[(size_t)rr * c->width + cc]);
        }
    }
    color_scale(acc, 1.0 / 9.0);
    c->color_space_fn(acc, res);
}

static uint16_t
quantize(double srgb, double srgb_max, double inverse)
{
    if (srgb > srgb_max) {
        return 65535;
    }
    if (srgb < 0) {
        return 0;
    }
    return (uint16_t)floor(srgb * inverse);
}

/*
 * One pixel's three 16-bit values: the scaling / clamp statements, rgb_to_srgb and quantize of the reference's
 * construct_ppm (canvas.c:150-327) and write_png (canvas.c:376-510). The only definition of that arithmetic: the
 * host pass calls it for every pixel, the device path (frt_encode.hip) for the values it left undecided.
 */
static void
encode_pixel(const Color px, int mode, const double srgb_max[3], const double inv[3], uint16_t q[3])
{
    Color t, s;
    memcpy(t, px, sizeof(Color));
    if (mode == FRT_ENCODE_PPM_SCALED) {
        double len = t[0] + t[1] + t[2];
        if (len > FRT_SQRT3) {
            color_scale(t, 1.0 / len);
            color_scale(t, FRT_SQRT3);
        }
    } else {
        for (int k = 0; k < 3; ++k) {
            if (t[k] > 1.0) {
                t[k] = 1.0;
            } else if (t[k] < 0) {
                t[k] = 0.0;
            }
        }
    }
    rgb_to_srgb(t, s);
    for (int k = 0; k < 3; ++k) {
        q[k] = quantize(s[k], srgb_max[k], inv[k]);
    }
}

/* pass 1: per-channel linear maximum (starts at 0) */
static void
host_rgb_max(const Color *arr, size_t npx, Color rgb_max)
{
    memset(rgb_max, 0, sizeof(Color));
    for (size_t i = 0; i < npx; ++i) {
        for (int k = 0; k < 3; ++k) {
            if (arr[i][k] > rgb_max[k]) {
                rgb_max[k] = arr[i][k];
            }
        }
    }
}

/* pass 2: maximum of sRGB(pixel / rgb_max) */
static void
host_srgb_max(const Color *arr, size_t npx, const Color rgb_max, Color srgb_max)
{
    memset(srgb_max, 0, sizeof(Color));
    for (size_t i = 0; i < npx; ++i) {
        Color t, s;
        memcpy(t, arr[i], sizeof(Color));
        t[0] /= rgb_max[0];
        t[1] /= rgb_max[1];
        t[2] /= rgb_max[2];
        rgb_to_srgb(t, s);
        for (int k = 0; k < 3; ++k) {
            if (s[k] > srgb_max[k]) {
                srgb_max[k] = s[k];
            }
        }
    }
}

/* construct_ppm's srgb_max by its two full passes (the device path takes rgb_to_srgb(1.0) instead: DESIGN.md
 * "Image encode"; tests/test_encode.py compares the two) */
void
frt_srgb_max_full(const double *rgba, size_t width, size_t height, double out[3])
{
    Color rgb_max, srgb_max;
    host_rgb_max((const Color *)rgba, width * height, rgb_max);
    host_srgb_max((const Color *)rgba, width * height, rgb_max, srgb_max);
    memcpy(out, srgb_max, 3 * sizeof(double));
}

static double
clock_ms(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec * 1e3 + (double)ts.tv_nsec * 1e-6;
}

/* the first device render_multi / frt_host_prepare last used in this process, -1 while none was: FRT_ENCODE=auto
 * takes the device only then (a process that only writes an image does not pay HIP's start-up for it) */
static int g_encode_device = -1;

void
frt_encode_note_device(int device)
{
    __atomic_store_n(&g_encode_device, device, __ATOMIC_RELAXED);
}

int
frt_encode_hint_device(void)
{
    return __atomic_load_n(&g_encode_device, __ATOMIC_RELAXED);
}

static _Thread_local frt_encode_stats t_encode_last;

void
frt_encode_last(frt_encode_stats *out)
{
    *out = t_encode_last;
}

size_t
frt_encode_stats_size(void)
{
    return sizeof(frt_encode_stats);
}

static const char *const decline_names[] = {"taken", "a channel's maximum is 0", "a non-finite pixel",
                                            "too many undecided values", "no usable device", "image too large"};

/* FRT_ENCODE=host | device | auto (default auto), read at every call */
static int
encode_backend_env(void)
{
    const char *e = getenv("FRT_ENCODE");
    if (e != NULL && strcmp(e, "host") == 0) {
        return FRT_ENCODE_HOST;
    }
    if (e != NULL && strcmp(e, "device") == 0) {
        return FRT_ENCODE_DEVICE;
    }
    return FRT_ENCODE_AUTO;
}

/* the reason the device would decline this canvas for, had there been one (the host pass reports it) */
static int
classify_canvas(const Color *arr, size_t npx, int mode, const Color rgb_max)
{
    for (size_t i = 0; i < npx; ++i) {
        for (int k = 0; k < 3; ++k) {
            if (!isfinite(arr[i][k])) {
                return FRT_ENCODE_NON_FINITE;
            }
        }
    }
    if (mode != FRT_ENCODE_PNG && (rgb_max[0] == 0.0 || rgb_max[1] == 0.0 || rgb_max[2] == 0.0)) {
        return FRT_ENCODE_ZERO_MAX;
    }
    return FRT_ENCODE_NO_DEVICE;
}

static void
put16(unsigned char *out, const uint16_t q)
{
    out[0] = (unsigned char)(q >> 8);
    out[1] = (unsigned char)(q & 0xFF);
}

/*
 * The 6 * width * height payload bytes of a canvas in host memory (arr) or device memory (dev_rgba, arr NULL).
 * print: construct_ppm's two print_color lines. Returns 0, or -1 when a device-resident canvas could not be
 * fetched for the host pass.
 */
static int
encode16(const Color *arr, const double *dev_rgba, size_t width, size_t height, int mode, int backend, int device,
         int print, unsigned char *out, frt_encode_stats *st)
{
    const size_t npx = width * height;
    const int hint = __atomic_load_n(&g_encode_device, __ATOMIC_RELAXED);
    memset(st, 0, sizeof(*st));
    st->values = 3 * (uint64_t)npx;
    st->mode = mode;
    st->device = -1;
    if (backend == FRT_ENCODE_AUTO) {
        backend = hint >= 0 ? FRT_ENCODE_DEVICE : FRT_ENCODE_HOST;
    }
    if (device < 0) {
        device = hint >= 0 ? hint : 0;
    }
    if (backend == FRT_ENCODE_DEVICE && npx > 0) {
        /* the quantiser's constants by the host's own arithmetic: with every rgb_max > 0 the pixel holding a
         * maximum gives x / x = 1.0 and no other quotient exceeds 1, so srgb_max is rgb_to_srgb(1.0) */
        const Color one = {1.0, 1.0, 1.0, 0.0};
        Color s_one;
        double srgb_max[4] = {1.0, 1.0, 1.0, 0.0}, inv[3] = {65535.0, 65535.0, 65535.0};
        unsigned short code_one[3];
        rgb_to_srgb(one, s_one);
        for (int k = 0; k < 3; ++k) {
            if (mode != FRT_ENCODE_PNG) {
                srgb_max[k] = s_one[k];
                inv[k] = 65535.0 / srgb_max[k];
            }
            code_one[k] = quantize(s_one[k], srgb_max[k], inv[k]);
        }
        const size_t cap = (size_t)(st->values / 64) + 1;
        uint32_t *und_idx = (uint32_t *)malloc(cap * sizeof(uint32_t));
        double *und_px = arr == NULL ? (double *)malloc(cap * sizeof(Color)) : NULL;
        int rc = -1;
        if (und_idx != NULL && (arr != NULL || und_px != NULL)) {
            rc = frt_encode16_device(arr != NULL ? (const double *)arr : dev_rgba, arr == NULL, width, height, mode,
                                     device, srgb_max, inv, code_one, out, und_idx, und_px, st);
        } else {
            st->decline = FRT_ENCODE_NO_DEVICE;
        }
        if (rc == 0) {
            const double p0 = clock_ms();
            for (uint64_t j = 0; j < st->undecided; ++j) {
                const size_t p = und_idx[j] / 3;
                const int k = (int)(und_idx[j] % 3);
                uint16_t q[3];
                encode_pixel(arr != NULL ? arr[p] : (const double *)(und_px + 4 * j), mode, srgb_max, inv, q);
                put16(out + 6 * p + 2 * k, q[k]);
            }
            st->patch_ms = clock_ms() - p0;
            if (print) {
                Color m = {st->rgb_max[0], st->rgb_max[1], st->rgb_max[2], 0.0};
                print_color(m);
                print_color(srgb_max);
            }
        }
        free(und_idx);
        free(und_px);
        if (rc == 0) {
            return 0;
        }
        fprintf(stderr, "frt: image encode falls back to the host pass: %s%s%s\n", decline_names[st->decline],
                rc < 0 ? ": " : "", rc < 0 ? frt_encode_error() : "");
    }

    /* the host pass: the reference's three passes */
    const int wanted_device = backend == FRT_ENCODE_DEVICE;
    const int decline = st->decline;
    Color *fetched = NULL;
    if (arr == NULL) {
        fetched = (Color *)malloc(npx * sizeof(Color));
        if (fetched == NULL || frt_encode_fetch(fetched, dev_rgba, npx * sizeof(Color), device) != 0) {
            free(fetched);
            return -1;
        }
        arr = fetched;
    }
    const double h0 = clock_ms();
    Color rgb_max = {0.0, 0.0, 0.0, 0.0}, srgb_max = {1.0, 1.0, 1.0, 0.0};
    double inv[3] = {65535.0, 65535.0, 65535.0};
    if (mode != FRT_ENCODE_PNG) {
        host_rgb_max(arr, npx, rgb_max);
        if (print) {
            print_color(rgb_max);
        }
        host_srgb_max(arr, npx, rgb_max, srgb_max);
        if (print) {
            print_color(srgb_max);
        }
        for (int k = 0; k < 3; ++k) {
            inv[k] = 65535.0 / srgb_max[k];
        }
    }
    for (size_t i = 0; i < npx; ++i) {
        uint16_t q[3];
        encode_pixel(arr[i], mode, srgb_max, inv, q);
        for (int k = 0; k < 3; ++k) {
            put16(out, q[k]);
            out += 2;
        }
    }
    const double host_ms = clock_ms() - h0;
    st->backend = FRT_ENCODE_HOST;
    st->undecided = 0;
    st->host_ms = host_ms;
    memcpy(st->rgb_max, rgb_max, 3 * sizeof(double));
    memcpy(st->srgb_max, srgb_max, 3 * sizeof(double));
    st->decline = !wanted_device ? FRT_ENCODE_TAKEN
                  : decline == FRT_ENCODE_NO_DEVICE ? classify_canvas(arr, npx, mode, rgb_max) : decline;
    free(fetched);
    return 0;
}

int
frt_encode16(const double *rgba, int rgba_on_device, size_t width, size_t height, int mode, int backend, int device,
             unsigned char *out, frt_encode_stats *st)
{
    frt_encode_stats local;
    if (mode < FRT_ENCODE_PPM_SCALED || mode > FRT_ENCODE_PNG || backend < FRT_ENCODE_HOST ||
        backend > FRT_ENCODE_AUTO) {
        return -1;
    }
    int rc = encode16(rgba_on_device ? NULL : (const Color *)rgba, rgba, width, height, mode, backend, device, 0, out,
                      &local);
    t_encode_last = local;
    if (st != NULL) {
        *st = local;
    }
    return rc;
}

static Ppm
construct_ppm_with(Canvas c, bool use_scaling, int backend)
{
    char header[32];
    int n = snprintf(header, sizeof(header), "P6\n%zu %zu\n65535\n", c->width, c->height);
    size_t npx = c->width * c->height;
    Ppm ppm = ppm_alloc(npx * 6 + (size_t)n + 1);
    unsigned char *out = ppm->arr;
    memcpy(out, header, (size_t)n);
    out += n;
    frt_encode_stats st;
    encode16(c->arr, NULL, c->width, c->height, use_scaling ? FRT_ENCODE_PPM_SCALED : FRT_ENCODE_PPM_CLAMPED, backend,
             -1, 1, out, &st);
    t_encode_last = st;
    out[npx * 6] = '\n';
    return ppm;
}

Ppm
construct_ppm(Canvas c, bool use_scaling)
{
    return construct_ppm_with(c, use_scaling, encode_backend_env());
}

static char *
with_suffix(const char *path, const char *suffix)
{
    size_t a = strlen(path), b = strlen(suffix);
    char *s = (char *)malloc(a + b + 1);
    memcpy(s, path, a);
    memcpy(s + a, suffix, b + 1);
    return s;
}

int
write_ppm_file(Canvas c, const bool use_scaling, const char *file_path)
{
    char *full = with_suffix(file_path, ".ppm");
    Ppm ppm = construct_ppm(c, use_scaling);
    FILE *f = fopen(full, "wb");
    int rc = 0;
    if (f == NULL) {
        fprintf(stderr, "frt: cannot open %s for writing\n", full);
        rc = 1;
    } else {
        fwrite(ppm->arr, 1, ppm->len, f);
        fclose(f);
    }
    ppm_free(ppm);
    free(full);
    return rc;
}

int
write_png(Canvas c, const char *file_name)
{
    /* 48-bit RGB, sRGB intent absolute, empty Title text, clamped linear -> sRGB
     * -> floor(x*65535) (reference canvas.c:376-510) */
    int code = 0;
    char *full = with_suffix(file_name, ".png");
    uint16_t *buffer = NULL;
    png_structp png = NULL;
    png_infop info = NULL;
    FILE *fp = fopen(full, "wb");
    if (fp == NULL) {
        code = 1;
        goto done;
    }
    png = png_create_write_struct(PNG_LIBPNG_VER_STRING, NULL, NULL, NULL);
    if (png == NULL) {
        code = 2;
        goto done;
    }
    info = png_create_info_struct(png);
    if (info == NULL) {
        code = 2;
        goto done;
    }
    if (setjmp(png_jmpbuf(png))) {
        code = 2;
        goto done;
    }
    png_init_io(png, fp);
    png_set_IHDR(png, info, (png_uint_32)c->width, (png_uint_32)c->height, 16, PNG_COLOR_TYPE_RGB,
                 PNG_INTERLACE_NONE, PNG_COMPRESSION_TYPE_BASE, PNG_FILTER_TYPE_BASE);
    png_set_sRGB(png, info, PNG_sRGB_INTENT_ABSOLUTE);
    png_text title;
    memset(&title, 0, sizeof(title));
    title.compression = PNG_TEXT_COMPRESSION_NONE;
    title.key = (png_charp) "Title";
    title.text = NULL;
    title.text_length = 0;
    png_set_text(png, info, &title, 1);
    png_write_info(png, info);

    size_t npx = c->width * c->height;
    buffer = (uint16_t *)malloc(npx * 3 * sizeof(uint16_t));
    {
        frt_encode_stats st;
        encode16(c->arr, NULL, c->width, c->height, FRT_ENCODE_PNG, encode_backend_env(), -1, 0,
                 (unsigned char *)buffer, &st);
        t_encode_last = st;
    }
    for (size_t row = 0; row < c->height; ++row) {
        png_write_row(png, (png_bytep)buffer + 3 * sizeof(uint16_t) * row * c->width);
    }
    png_write_end(png, NULL);

done:
    if (fp) fclose(fp);
    if (info) png_free_data(png, info, PNG_FREE_ALL, -1);
    if (png) png_destroy_write_struct(&png, &info);
    free(buffer);
    free(full);
    return code;
}

void
construct_canvas_from_ppm_file(Canvas *c, const char *file_path, bool super_sample, void (*color_space_fn)(const Color, Color))
{
    /* ASCII sample values after a "P6"-style header (reference canvas.c:330-365) */
    char magic[32];
    size_t w, h, maxv;
    FILE *f = fopen(file_path, "r");
    if (f == NULL) {
        printf("Error opening file %s", file_path);
        return;
    }
    if (fscanf(f, "%31s %zu %zu %zu", magic, &w, &h, &maxv) != 4) {
        fclose(f);
        return;
    }
    *c = canvas_alloc(w, h, super_sample, color_space_fn);
    for (size_t i = 0; i < w * h; ++i) {
        unsigned int v[3] = {0, 0, 0};
        for (int k = 0; k < 3; ++k) {
            if (fscanf(f, "%u", &v[k]) != 1) {
                v[k] = 0;
            }
            (*c)->arr[i][k] = (double)v[k] / (double)maxv;
        }
        (*c)->arr[i][3] = 0.0;
    }
    fclose(f);
}

int
read_png(Canvas *c, const char *filename, bool super_sample, void (*color_space_fn)(const Color, Color))
{
    int code = 0;
    png_structp png = NULL;
    png_infop info = NULL;
    png_bytep *rows = NULL;
    unsigned char *buffer = NULL;
    FILE *fp = fopen(filename, "rb");
    if (fp == NULL) {
        code = 1;
        goto done;
    }
    png = png_create_read_struct(PNG_LIBPNG_VER_STRING, NULL, NULL, NULL);
    if (png == NULL) {
        code = 2;
        goto done;
    }
    info = png_create_info_struct(png);
    if (info == NULL) {
        code = 2;
        goto done;
    }
    if (setjmp(png_jmpbuf(png))) {
        code = 2;
        goto done;
    }
    png_init_io(png, fp);
    png_read_info(png, info);
    png_byte color_type = png_get_color_type(png, info);
    png_byte depth = png_get_bit_depth(png, info);
    size_t w = png_get_image_width(png, info);
    size_t h = png_get_image_height(png, info);
    if (color_type == PNG_COLOR_TYPE_PALETTE) png_set_palette_to_rgb(png);
    if (color_type == PNG_COLOR_TYPE_GRAY && depth < 8) png_set_expand_gray_1_2_4_to_8(png);
    if (color_type == PNG_COLOR_TYPE_GRAY || color_type == PNG_COLOR_TYPE_GRAY_ALPHA) png_set_gray_to_rgb(png);
    if (color_type & PNG_COLOR_MASK_ALPHA) png_set_strip_alpha(png);
    png_read_update_info(png, info);

    size_t bytes_per_sample = depth == 16 ? 2 : 1;
    rows = (png_bytep *)malloc(h * sizeof(png_bytep));
    buffer = (unsigned char *)malloc(w * h * 3 * bytes_per_sample);
    for (size_t i = 0; i < h; ++i) {
        rows[i] = buffer + 3 * i * w * bytes_per_sample;
    }
    png_read_image(png, rows);

    *c = canvas_alloc(w, h, super_sample, color_space_fn);
    const unsigned char *p = buffer;
    for (size_t i = 0; i < w * h; ++i) {
        Color *o = (*c)->arr + i;
        (*o)[3] = 0.0;
        if (depth == 16) {
            for (int k = 0; k < 3; ++k) {
                uint16_t v = (uint16_t)(((p[2 * k] & 0xff) << 8) | (p[2 * k + 1] & 0xff));
                (*o)[k] = (double)v / 65535.0;
            }
            p += 6;
        } else {
            for (int k = 0; k < 3; ++k) {
                (*o)[k] = (double)p[k] / 255.0;
            }
            p += 3;
        }
    }

done:
    if (fp) fclose(fp);
    if (info) png_free_data(png, info, PNG_FREE_ALL, -1);
    if (png) png_destroy_read_struct(&png, &info, NULL);
    free(rows);
    free(buffer);
    return code;
}

/* Encode a raw rgba canvas (width*height*4 doubles) exactly as write_ppm_file
 * would; used by tests and bench.py to compare PPM bytes without touching the
 * file system. Returns the byte count, writes into out when it is large enough. */
size_t
frt_encode_ppm(const double *rgba, size_t width, size_t height, int use_scaling, unsigned char *out, size_t cap)
{
    struct canvas c;
    c.arr = (Color *)rgba;
    c.width = width;
    c.height = height;
    c.super_sample = false;
    c.color_space_fn = NULL;
    Ppm p = construct_ppm_with(&c, use_scaling != 0, FRT_ENCODE_HOST);
    size_t n = p->len;
    if (out != NULL && cap >= n) {
        memcpy(out, p->arr, n);
    }
    ppm_free(p);
    return n;
}
