// ct_hostpath.cpp — the per-module host loops of compress_modules / decompress_modules, in C++ (CPython extension `_hostpath`), for every format that has
// a table launch: pack-quantized W4 (w4_*), the plain 8-bit codecs (q8_*), mxfp8 (mx8_*), pack-quantized W8 (w8_*, finished by the W4 functions), NVFP4 /
// MXFP4 (fp4_*) — and, launching per module by address, pack-quantized in the other word widths and with activation ordering (wb_*).
//
// Why: compress_model / decompress_model of a 154-module checkpoint spend 20 us of interpreter time per module and direction in
// PackedQuantizationCompressor.compress_modules / decompress_modules (dictionary look-ups, ~25 tensor attribute calls, torch.empty,
// nn.Parameter, dictionary surgery) next to two kernels of 0.42 ms each (bench.py `tinyllama_checkpoint.api`).  The same steps here
// cost ~5 us.  Nothing in this file computes on tensor data: it reads the modules' own `_parameters`, validates layouts, allocates
// outputs with ATen, fills the `struct ct_w4_item` table (include/ct_hip.h) that the `ct_*_batch` launches consume, and — after the Python side
// (compressors/base.py:run_planned) has planned, uploaded and LAUNCHED the table — rewrites the modules' parameter
// dictionaries under the running kernel, exactly as compressed_tensors_amd/utils/module.py:swap_direct_entries does
// (reference: compressors/base.py:95-131, utils/module.py:33-65, compressors/pack_quantized/base.py:62-163).
//
// How the loops are laid out: ONE driver walks the modules (`each_plain_module`: the `infos`, the plain-class test, the module's
// dictionaries, the hand-back in `rest`), ONE plan driver on top of it collects tables (`plan_modules`: the batch map, its way back to Python), ONE row builder
// fills a table row by the struct's field names (`item_row`), ONE finish driver walks the jobs (`finish_jobs`).  A scheme supplies a TAKE function
// `(module, info, Entries&, Sink&) -> bool` — is the module this scheme's plain case?  then allocate, hand the sink the row(s) and the job — and the
// dictionary surgery of its finish.  Tests a loop shares with the others are named functions (`dense_source`, `stored_shape`, `Sink::at`, `drop_mask_names`);
// what a loop asks beyond them stands next to the shared call.
//
// Also here (second half of the file): the host side of the two plug-in calls that wait for the device before they return — the
// sparse-bitmask compress and the default mode of the marlin-24 compress — where the interpreter's 15-20 us sat in series with a
// 30-42 us kernel.
//
// A module that is anything but the plain case (a buffer among its entries, a trainable parameter that stays, a class with its own
// __setattr__, activation arguments, an unusual layout) is handed back untouched in `rest`; the Python path,
// which covers every case, takes it.  The Python path is also what runs when this extension has not been built.
#include "ct_hip.h"  // struct ct_w4_item: the table row (the build passes -I include)

#include <torch/csrc/autograd/python_variable.h>
#include <torch/extension.h>

#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <optional>
#include <pybind11/stl.h>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

namespace py = pybind11;

namespace {

// (raw pointers, referenced once at import and never released: a py::object at namespace scope would be destroyed after the interpreter)
PyObject* g_make_subclass = nullptr;   // torch.Tensor._make_subclass
PyObject* g_parameter_cls = nullptr;   // torch.nn.Parameter
PyObject* g_module_setattr = nullptr;  // torch.nn.Module.__setattr__
PyObject* g_module_delattr = nullptr;  // torch.nn.Module.__delattr__
struct PlainEntry { bool plain; unsigned int tag; };
std::unordered_map<PyTypeObject*, PlainEntry> g_plain_type;
// One thread-local word, touched on purpose (module init and every entry point).  glibc before 2.39 (BZ #19924; this image: 2.35): after a dlopen
// of ANY library that carries a TLS segment, every `__tls_get_addr` of a thread — PyTorch makes dozens per tensor it creates or releases — takes the
// dynamic linker's slow path until that thread has touched the TLS of the NEWEST such library; a process that has imported torch and friends is usually
// in that state, and stays in it.  This extension is imported lazily, at the first call that needs it, normally after everything else has been loaded:
// touching its own TLS then puts the calling thread back on the fast path.  Measured on the 154-module checkpoint:
// w4_finish_compress / w4_finish_decompress — the functions that release and create tensors — 20-25 % faster, and the reason a build of this file
// without -DNDEBUG (pybind11 then counts references in a thread_local) was FASTER than one with it, and faster imported late than early.
thread_local volatile int64_t g_tls_touch = 0;
inline void touch_tls() { g_tls_touch = g_tls_touch + 1; }

bool g_allow_cpu = false;  // tests only (tests/test_host_logic.py): run the host logic on CPU tensors, with the launch stubbed out

struct Names {
    PyObject *parameters, *buffers, *weight, *weight_scale, *weight_zero_point, *weight_g_idx, *weight_packed, *weight_shape, *quantization_status,
        *setattr, *delattr;
    void init() {
        parameters = PyUnicode_InternFromString("_parameters");
        buffers = PyUnicode_InternFromString("_buffers");
        weight = PyUnicode_InternFromString("weight");
        weight_scale = PyUnicode_InternFromString("weight_scale");
        weight_zero_point = PyUnicode_InternFromString("weight_zero_point");
        weight_g_idx = PyUnicode_InternFromString("weight_g_idx");
        weight_packed = PyUnicode_InternFromString("weight_packed");
        weight_shape = PyUnicode_InternFromString("weight_shape");
        quantization_status = PyUnicode_InternFromString("quantization_status");
        setattr = PyUnicode_InternFromString("__setattr__");
        delattr = PyUnicode_InternFromString("__delattr__");
    }
} N;

// does the module's class keep nn.Module's own attribute hooks?  (then writing `_parameters` directly cannot be told from setattr)
bool plain_type(PyObject* module) {
    PyTypeObject* tp = Py_TYPE(module);
    // keyed by the type object, which the table keeps alive (a freed type's address can be reused by another class), and validated by the
    // type's version tag: CPython invalidates it whenever the class or one of its bases is modified (a later `Cls.__setattr__ = ...`)
    const bool tagged = (tp->tp_flags & Py_TPFLAGS_VALID_VERSION_TAG) != 0;
    auto it = g_plain_type.find(tp);
    if (it != g_plain_type.end() && tagged && it->second.tag == tp->tp_version_tag) return it->second.plain;
    PyObject* s = PyObject_GetAttr(reinterpret_cast<PyObject*>(tp), N.setattr);  // (the lookup assigns a fresh version tag)
    PyObject* d = PyObject_GetAttr(reinterpret_cast<PyObject*>(tp), N.delattr);
    const bool plain = s && d && s == g_module_setattr && d == g_module_delattr;
    Py_XDECREF(s);
    Py_XDECREF(d);
    PyErr_Clear();
    const unsigned int tag = (tp->tp_flags & Py_TPFLAGS_VALID_VERSION_TAG) ? tp->tp_version_tag : 0u;
    if (it == g_plain_type.end()) {
        Py_INCREF(tp);
        g_plain_type.emplace(tp, PlainEntry{plain, tag});
    } else {
        it->second = PlainEntry{plain, tag};
    }
    return plain;
}

// an attribute the way `getattr(obj, name, None)` finds it for names that live in the instance dictionary or on the class, WITHOUT falling into
// nn.Module.__getattr__ on a miss (a Python-level search of _parameters / _buffers / _modules that then raises: ~2 us for every container
// module of a model walk).  New reference or nullptr.
PyObject* lookup_plain(PyObject* obj, PyObject* name) {
    PyObject** dictptr = _PyObject_GetDictPtr(obj);
    if (dictptr && *dictptr) {
        PyObject* v = PyDict_GetItem(*dictptr, name);  // borrowed
        if (v) {
            Py_INCREF(v);
            return v;
        }
    }
    PyObject* t = _PyType_Lookup(Py_TYPE(obj), name);  // borrowed; a plain class attribute or a descriptor
    if (!t) return nullptr;
    descrgetfunc get = Py_TYPE(t)->tp_descr_get;
    if (get) {
        PyObject* v = get(t, obj, reinterpret_cast<PyObject*>(Py_TYPE(obj)));
        if (!v) PyErr_Clear();
        return v;
    }
    Py_INCREF(t);
    return t;
}

// infos: a list with one integer per module, or a callable scheme -> integer that is asked once per distinct scheme object
struct Infos {
    PyObject* src;
    bool callable;
    PyObject* scheme_name = PyUnicode_InternFromString("quantization_scheme");
    std::unordered_map<PyObject*, int64_t> cache;
    explicit Infos(PyObject* s) : src(s), callable(!PyList_Check(s)) {}
    int64_t of(PyObject* module, Py_ssize_t i) {
        if (!callable) return PyLong_AsLongLong(PyList_GET_ITEM(src, i));
        PyObject* scheme = lookup_plain(module, scheme_name);
        if (!scheme) return -1;
        auto it = cache.find(scheme);
        int64_t v;
        if (it != cache.end()) v = it->second;
        else {
            PyObject* r = PyObject_CallFunctionObjArgs(src, scheme, nullptr);
            if (!r) {
                Py_DECREF(scheme);
                throw py::error_already_set();
            }
            v = PyLong_AsLongLong(r);
            Py_DECREF(r);
            cache.emplace(scheme, v);  // (the module keeps the scheme alive for the duration of the call)
        }
        Py_DECREF(scheme);
        return v;
    }
};

struct Entries {
    PyObject* params = nullptr;   // new references
    PyObject* buffers = nullptr;
    ~Entries() {
        Py_XDECREF(params);
        Py_XDECREF(buffers);
    }
    bool open(PyObject* module) {
        params = PyObject_GetAttr(module, N.parameters);
        buffers = PyObject_GetAttr(module, N.buffers);
        if (!params || !buffers || !PyDict_Check(params) || !PyDict_Check(buffers)) {
            PyErr_Clear();
            return false;
        }
        return true;
    }
    // a parameter entry as a tensor, nullptr when absent / None / not a tensor
    const at::Tensor* tensor(PyObject* name) const {
        PyObject* o = PyDict_GetItem(params, name);  // borrowed
        if (!o || o == Py_None || !THPVariable_Check(o)) return nullptr;
        return &THPVariable_Unpack(o);
    }
    bool has(PyObject* name) const { return PyDict_GetItem(params, name) != nullptr; }
};

PyObject* g_input_zero_point = nullptr;   // entry names beyond `Names` (interned at import)
PyObject* g_output_zero_point = nullptr;
PyObject* g_weight_global_scale = nullptr;

inline bool aligned(const at::Tensor& t, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(t.data_ptr()) & (bytes - 1)) == 0; }
inline bool aligned16(const at::Tensor& t) { return aligned(t, 16); }
inline bool half_type(at::ScalarType t) { return t == at::kBFloat16 || t == at::kHalf; }
inline int half_code(at::ScalarType t) { return t == at::kHalf ? 1 : 2; }  // _lib.F16 / _lib.BF16

// C ABI element code of a tensor's dtype (include/ct_hip.h enum ct_dtype), -1 for a type the ABI has no code for
int dtype_code(at::ScalarType t) {
    switch (t) {
        case at::kFloat: return CT_F32;
        case at::kHalf: return CT_F16;
        case at::kBFloat16: return CT_BF16;
        case at::kChar: return CT_I8;
        case at::kInt: return CT_I32;
        case at::kByte: case at::kBool: return CT_U8;
        case at::kShort: return CT_I16;
        case at::kLong: return CT_I64;
        default: return -1;
    }
}

// the dense-source test every loop makes of the tensor its launch streams (weights, codes or packed words): two-dimensional, contiguous, on a GPU — on
// GPU `device_index` where the loop launches on one device — and aligned to what the kernel loads at once
inline bool dense_source(const at::Tensor& t, uintptr_t align = 16, int device_index = -1) {
    return ((t.is_cuda() && (device_index < 0 || t.device().index() == device_index)) || g_allow_cpu) && t.is_contiguous() && aligned(t, align) && t.dim() == 2;
}

// an optional entry as the loops want it: a tensor (`t`, what Entries::tensor found under `name`) or not there at all — not None, not another object
inline bool tensor_or_absent(const Entries& e, const at::Tensor* t, PyObject* name) { return t != nullptr || !e.has(name); }

inline const void* data_or_null(const at::Tensor* t) { return t ? t->data_ptr() : nullptr; }

// the stored `weight_shape` of a pack-quantized module as upstream writes it (int64, CPU, two elements: pack_quantized/base.py:105): its rows and
// columns, or false for anything else
bool stored_shape(const at::Tensor* shape_t, int64_t& rows, int64_t& cols) {
    if (!shape_t || !shape_t->device().is_cpu() || shape_t->scalar_type() != at::kLong || shape_t->numel() != 2 || !shape_t->is_contiguous()) return false;
    rows = shape_t->data_ptr<int64_t>()[0];
    cols = shape_t->data_ptr<int64_t>()[1];
    return rows > 0 && cols > 0;
}

// the drop mask of the `infos` encodings: the zero points a symmetric scheme does not store (compressors/base.py: zp_drop_mask), bit k = name k
inline std::array<PyObject*, 3> drop_mask_names() { return {N.weight_zero_point, g_input_zero_point, g_output_zero_point}; }

// every parameter that stays must already be a non-trainable Parameter (else the generic path re-wraps it); no buffers at all.  Leaving: the names in
// `leaving` and the zero points of `dropmask`
bool staying_entries_are_final(const Entries& e, std::initializer_list<PyObject*> leaving, int dropmask = 0) {
    if (PyDict_Size(e.buffers) != 0) return false;
    const auto dropped = drop_mask_names();
    PyObject *key, *value;
    Py_ssize_t pos = 0;
    while (PyDict_Next(e.params, &pos, &key, &value)) {
        bool leaves = false;
        for (PyObject* l : leaving) leaves = leaves || key == l || PyObject_RichCompareBool(key, l, Py_EQ) == 1;
        for (int k = 0; k < 3; ++k)
            if ((dropmask >> k) & 1) leaves = leaves || key == dropped[k] || PyObject_RichCompareBool(key, dropped[k], Py_EQ) == 1;
        if (leaves || value == Py_None) continue;
        if (!THPVariable_Check(value) || THPVariable_Unpack(value).requires_grad()) return false;
    }
    return true;
}

py::object make_parameter(const at::Tensor& t) {  // == torch.nn.Parameter(t, requires_grad=False) for a plain tensor
    py::object wrapped = py::reinterpret_steal<py::object>(THPVariable_Wrap(t));
    PyObject* r = PyObject_CallFunctionObjArgs(g_make_subclass, g_parameter_cls, wrapped.ptr(), Py_False, nullptr);
    if (!r) throw py::error_already_set();
    return py::reinterpret_steal<py::object>(r);
}

void set_entry(const Entries& e, PyObject* name, const at::Tensor& t) { PyDict_SetItem(e.params, name, make_parameter(t).ptr()); }  // in place when the key exists

void drop(PyObject* dict, PyObject* name) {  // del dict[name] if present
    if (PyDict_GetItem(dict, name) && PyDict_DelItem(dict, name) != 0) PyErr_Clear();
}

void drop_zero_points(const Entries& e, long dropmask) {
    const auto names = drop_mask_names();
    for (int k = 0; k < 3; ++k)
        if ((dropmask >> k) & 1) drop(e.params, names[k]);
}

void set_status(PyObject* module, PyObject* status) {
    PyObject** dictptr = _PyObject_GetDictPtr(module);
    if (dictptr && *dictptr) PyDict_SetItem(*dictptr, N.quantization_status, status);  // a plain attribute: what nn.Module.__setattr__ ends up doing
    else PyObject_SetAttr(module, N.quantization_status, status);
}

bool dict_has(PyObject* module, PyObject* name) {
    PyObject** dictptr = _PyObject_GetDictPtr(module);
    return dictptr && *dictptr && PyDict_GetItem(*dictptr, name) != nullptr;
}

inline py::object borrowed(PyObject* o) { return py::reinterpret_borrow<py::object>(o); }
inline py::object wrap(const at::Tensor& t) { return py::reinterpret_steal<py::object>(THPVariable_Wrap(t)); }
// a module's own entry object, for a job: it keeps the tensor alive until the launch has been issued (the table holds raw pointers); None when absent
inline py::object entry_ref(const Entries& e, PyObject* name) {
    PyObject* o = PyDict_GetItem(e.params, name);
    return o ? borrowed(o) : py::none();
}

// ------------------------------------------------------------------------------------------
// The table, its row builder and the drivers
// ------------------------------------------------------------------------------------------
static_assert(sizeof(ct_w4_item) % sizeof(int64_t) == 0, "a table row is a whole number of 64-bit words");
constexpr int kItemWords = sizeof(ct_w4_item) / sizeof(int64_t);  // the Python side reads the same struct (codec._ITEM_WORDS, codec.item_row)

// one row of a table, by the struct's field names; everything else (the fields ct_*_batch_plan derives) zero.  What the fields MEAN is the launch's
// business (include/ct_hip.h: every `ct_*_batch` entry says how it reads struct ct_w4_item).
ct_w4_item item_row(const void* src, const void* scale, const void* zp, void* dst, int64_t rows, int64_t cols, int64_t group, void* zp_packed = nullptr) {
    ct_w4_item it{};
    it.src = src;
    it.scale = scale;
    it.zp = zp;
    it.dst = dst;
    it.rows = rows;
    it.cols = cols;
    it.group = group;
    it.zp_packed = zp_packed;
    return it;
}

struct Batch {
    std::vector<int64_t> words;      // kItemWords per item: struct ct_w4_item
    std::vector<int64_t> aux_words;  // the same layout: the table of the launch that goes with the weights' — the zero points of ASYMMETRIC W4 modules whose
                                     // weights' launch cannot take them in packed form (ct_zp4_pack_dim0_batch), the scales of mxfp8 (ct_mx_scale_batch)
    py::list jobs;
    int n = 0, aux_n = 0;
    static void append(std::vector<int64_t>& to, const ct_w4_item& it) {
        to.resize(to.size() + kItemWords);
        std::memcpy(to.data() + to.size() - kItemWords, &it, sizeof(it));
    }
    void row(const ct_w4_item& it) { append(words, it), n += 1; }
    void aux_row(const ct_w4_item& it) { append(aux_words, it), aux_n += 1; }
};

// where a take function puts what it planned: one Batch per (device index or -1 for the tests' CPU tensors, the launch's code — what the code encodes is
// between the take function and its Python launcher).  std::map: the batches leave in key order, which is launch order.
struct Sink {
    std::map<std::pair<int, int>, Batch> batches;
    Batch& at(const at::Tensor& t, int code) { return batches[{t.is_cuda() ? (int)t.device().index() : -1, code}]; }
};

at::Tensor words_tensor(const std::vector<int64_t>& v) {
    at::Tensor t = at::empty({(int64_t)v.size()}, at::TensorOptions().dtype(at::kLong));
    if (!v.empty()) std::memcpy(t.data_ptr(), v.data(), v.size() * sizeof(int64_t));
    return t;
}

py::dict batches_to_python(const Sink& sink) {  // {(device, code): (words, n, jobs, aux words, aux n)}: what compressors/base.py:run_planned iterates
    py::dict out;
    for (auto& kv : sink.batches) {
        const Batch& b = kv.second;
        out[py::make_tuple(kv.first.first, kv.first.second)] = py::make_tuple(words_tensor(b.words), b.n, b.jobs, words_tensor(b.aux_words), b.aux_n);
    }
    return out;
}

// The loop head and the refusal tail of every module loop.  `infos` (nullptr: the loop has none, every module's info is 1) as `Infos` reads it;
// `body(module, info, entries) -> bool` sees a module of a plain class with its dictionaries open and answers whether it took it.  Every other module —
// in module order — is the list returned: the Python path's.
template <class Body>
py::list each_plain_module(const py::list& modules, PyObject* infos_arg, Body body) {
    touch_tls();
    py::list rest;
    std::optional<Infos> infos;
    if (infos_arg) infos.emplace(infos_arg);
    const Py_ssize_t n = PyList_GET_SIZE(modules.ptr());
    for (Py_ssize_t i = 0; i < n; ++i) {
        PyObject* m = PyList_GET_ITEM(modules.ptr(), i);
        const int64_t info = infos ? infos->of(m, i) : 1;
        Entries e;
        if (!(plain_type(m) && e.open(m) && body(m, info, e))) rest.append(borrowed(m));
    }
    return rest;
}

// The plan driver.  `take(module, info, entries, sink) -> bool`: false = not this scheme's plain case, and then NOTHING was put into the sink; true = the
// outputs are allocated and the sink's batch for the module holds its row (rows) and its job — a tuple that starts with the module, carries what the
// scheme's finish needs, and holds a reference to every INPUT the rows point at.  Returns (batches for Python, rest).
template <class Take>
py::tuple plan_modules(const py::list& modules, PyObject* infos_arg, Take take) {
    Sink sink;
    py::list rest = each_plain_module(modules, infos_arg, [&](PyObject* m, int64_t info, Entries& e) { return take(m, info, e, sink); });
    return py::make_tuple(batches_to_python(sink), rest);
}

// The finish driver, after the launch: `rewrite(job, entries)` is the dictionary surgery of one module (job[0]), then the module's status.
template <class Rewrite>
void finish_jobs(const py::list& jobs, PyObject* status, Rewrite rewrite) {
    touch_tls();
    const Py_ssize_t n = PyList_GET_SIZE(jobs.ptr());
    for (Py_ssize_t i = 0; i < n; ++i) {
        PyObject* job = PyList_GET_ITEM(jobs.ptr(), i);
        PyObject* m = PyTuple_GET_ITEM(job, 0);
        Entries e;
        if (!e.open(m)) throw std::runtime_error("module lost its _parameters");
        rewrite(job, e);
        set_status(m, status);
    }
}

inline const at::Tensor& job_tensor(PyObject* job, int k) { return THPVariable_Unpack(PyTuple_GET_ITEM(job, k)); }

at::Tensor shape_tensor(int64_t rows, int64_t cols) {  // `weight_shape`: int64, CPU, as upstream (pack_quantized/base.py:105)
    at::Tensor shape = at::empty({2}, at::TensorOptions().dtype(at::kLong));
    shape.data_ptr<int64_t>()[0] = rows;
    shape.data_ptr<int64_t>()[1] = cols;
    return shape;
}

// ------------------------------------------------------------------------------------------
// pack-quantized W4 (int4, 16-bit weights and scales of one dtype; ct_quant_pack_batch / ct_unpack_dequant_batch).  batch key code: the dtype code.
// compress infos[i]: group size of module i's scheme (0 = channel-wise), + kAsymmetric when the scheme stores packed zero points
// (pack_to_int32(zp, 4, packed_dim=0), pack_quantized/base.py:107-110), or < 0 when the scheme is not an int4 group / channel scheme
// ------------------------------------------------------------------------------------------
constexpr int64_t kAsymmetric = int64_t(1) << 40;

bool w4_take_compress(PyObject* m, int64_t info, Entries& e, Sink& sink) {
    const bool asym = info >= kAsymmetric;
    const int64_t ginfo = asym ? info - kAsymmetric : info;
    if (ginfo < 0 || dict_has(m, N.weight_packed) || dict_has(m, N.weight_shape)) return false;
    const at::Tensor *w = e.tensor(N.weight), *scale = e.tensor(N.weight_scale), *zp = e.tensor(N.weight_zero_point);
    // (the kernel loads scales and zero points in 16-byte units too: both aligned, unlike the per-module launches of the wb loop)
    if (!(w && scale && !e.has(N.weight_g_idx) && tensor_or_absent(e, zp, N.weight_zero_point) && dense_source(*w) && half_type(w->scalar_type()) &&
          scale->scalar_type() == w->scalar_type() && scale->is_contiguous() && aligned16(*scale) && scale->device() == w->device()))
        return false;
    const int64_t rows = w->size(0), cols = w->size(1), group = ginfo == 0 ? cols : ginfo;
    if (!(rows > 0 && cols % 32 == 0 && group % 32 == 0 && cols % group == 0 && scale->dim() == 2 && scale->size(0) == rows && scale->size(1) == cols / group)) return false;
    if (zp && !(zp->scalar_type() == at::kChar && zp->sizes() == scale->sizes() && zp->is_contiguous() && aligned16(*zp) && zp->device() == w->device())) return false;
    if (!((zp || !asym) && staying_entries_are_final(e, {N.weight, N.weight_zero_point}))) return false;
    at::Tensor packed = at::empty({rows, cols / 8}, w->options().dtype(at::kInt));
    at::Tensor zpp;  // int8 (R, G) -> int32 (ceil(R / 8), G): written by tail workgroups of the weights' own launch (ct_w4_item.zp_packed)
    if (asym) zpp = at::empty({(rows * 4 + 31) / 32, zp->size(1)}, w->options().dtype(at::kInt));
    Batch& b = sink.at(*w, half_code(w->scalar_type()));
    b.row(item_row(w->data_ptr(), scale->data_ptr(), data_or_null(zp), packed.data_ptr(), rows, cols, group, asym ? zpp.data_ptr() : nullptr));
    // (module, packed, rows, cols, keep-alive weight, zp_packed or None, keep-alive zero point or None)
    b.jobs.append(py::make_tuple(borrowed(m), wrap(packed), rows, cols, entry_ref(e, N.weight), asym ? wrap(zpp) : py::none(),
                                 asym ? entry_ref(e, N.weight_zero_point) : py::none()));
    return true;
}

// `weight` (and the zero point a symmetric scheme does not store) leave, `weight_packed` and `weight_shape` arrive, an asymmetric
// scheme's zero point is replaced by its packed form
void w4_finish_compress(py::list jobs, py::object status) {
    finish_jobs(jobs, status.ptr(), [](PyObject* job, Entries& e) {
        const int64_t rows = PyLong_AsLongLong(PyTuple_GET_ITEM(job, 2)), cols = PyLong_AsLongLong(PyTuple_GET_ITEM(job, 3));
        PyObject* zp_packed = PyTuple_GET_ITEM(job, 5);
        drop(e.params, N.weight);
        if (zp_packed == Py_None) drop(e.params, N.weight_zero_point);  // a symmetric scheme stores none (compressors/base.py: symmetric_zp_keys)
        set_entry(e, N.weight_packed, job_tensor(job, 1));
        set_entry(e, N.weight_shape, shape_tensor(rows, cols));
        if (zp_packed != Py_None) set_entry(e, N.weight_zero_point, THPVariable_Unpack(zp_packed));  // in place: same position
    });
}

// decompress infos[i]: 1 when module i's scheme is a symmetric int4 scheme (the strategy is inferred from the scale's shape, as `dequantize` does), 2 when
// it is an asymmetric int4 group / channel scheme (zero points stored packed along rows), else 0
bool w4_take_decompress(PyObject* m, int64_t info, Entries& e, Sink& sink) {
    const bool asym = info == 2;
    if (!(info == 1 || info == 2) || dict_has(m, N.weight)) return false;
    const at::Tensor *packed = e.tensor(N.weight_packed), *scale = e.tensor(N.weight_scale), *zpp = e.tensor(N.weight_zero_point);
    int64_t rows = 0, cols = 0;
    if (!(packed && scale && !e.has(N.weight_g_idx) && (asym ? zpp != nullptr : !e.has(N.weight_zero_point)) && !e.has(N.weight) && dense_source(*packed) &&
          packed->scalar_type() == at::kInt && scale->dim() == 2 && half_type(scale->scalar_type()) && scale->is_contiguous() && aligned16(*scale) &&
          scale->device() == packed->device() && stored_shape(e.tensor(N.weight_shape), rows, cols)))
        return false;
    if (!(scale->size(1) > 0 && cols % scale->size(1) == 0)) return false;
    const int64_t group = scale->size(1) == 1 ? cols : cols / scale->size(1);  // (R, 1): channel; (R, G): group (forward.py:99-130)
    if (!(cols % 32 == 0 && group % 32 == 0 && cols % group == 0 && scale->size(0) == rows && scale->size(1) == cols / group && packed->size(0) == rows &&
          packed->size(1) == cols / 8 && staying_entries_are_final(e, {N.weight_packed, N.weight_zero_point})))
        return false;
    if (asym && !(zpp->scalar_type() == at::kInt && zpp->dim() == 2 && zpp->size(0) == (rows * 4 + 31) / 32 && zpp->size(1) == scale->size(1) && zpp->is_contiguous() &&
                  zpp->device() == packed->device()))
        return false;
    at::Tensor out = at::empty({rows, cols}, scale->options());
    Batch& b = sink.at(*packed, half_code(scale->scalar_type()));
    at::Tensor zp;
    void* zpp_in = nullptr;
    if (asym) {
        zp = at::empty({rows, scale->size(1)}, packed->options().dtype(at::kChar));
        if (group == 128 && cols % 512 == 0 && rows * (cols / 8) < (int64_t(1) << 31) && aligned16(*zpp)) {
            // the weights' launch reads the zero points in their stored form and its tail workgroups write the int8 form back
            // (include/ct_hip.h, ct_w4_item.zp_packed) — no launch in front of it
            zpp_in = zpp->data_ptr();
        } else {  // int32 (ceil(R / 8), G) -> int8 (R, G): unpacked by the launch that runs BEFORE the weights' (the table below points at it)
            b.aux_row(item_row(zpp->data_ptr(), nullptr, nullptr, zp.data_ptr(), rows, scale->size(1), 0));
        }
    }
    b.row(item_row(packed->data_ptr(), scale->data_ptr(), asym ? zp.data_ptr() : nullptr, out.data_ptr(), rows, cols, group, zpp_in));
    // (module, out, keep-alive packed, unpacked zero points or None, keep-alive packed zero points or None)
    b.jobs.append(py::make_tuple(borrowed(m), wrap(out), entry_ref(e, N.weight_packed), asym ? wrap(zp) : py::none(),
                                 asym ? entry_ref(e, N.weight_zero_point) : py::none()));
    return true;
}

void w4_finish_decompress(py::list jobs, py::object status) {
    finish_jobs(jobs, status.ptr(), [](PyObject* job, Entries& e) {
        PyObject* zp = PyTuple_GET_ITEM(job, 3);
        drop(e.params, N.weight_packed);
        set_entry(e, N.weight, job_tensor(job, 1));
        if (zp != Py_None) set_entry(e, N.weight_zero_point, THPVariable_Unpack(zp));  // unpacked, int8, in place
    });
}

// ------------------------------------------------------------------------------------------
// 8-bit codecs (naive- / int- / float-quantized, reference compressors/naive_quantized/base.py:48-126): the same split — plan the table of
// `ct_q8_quant_batch` / `ct_q8_dequant_batch` from the modules' own entries, launch, rewrite the dictionaries under the kernel.  Mirrors
// NaiveQuantizationCompressor._batch_compress / _batch_decompress and codec.q8_batch_group (the Python loop: 7-9 us per module and direction, which a
// 1B-parameter FP8 checkpoint's modules do not hide).
// compress infos[i]: group_size (bits 0-19; 0 = none; the block width of a block scheme) | num_bits << 20 | FLOAT << 24 | strategy << 25 (0 tensor, 1 channel,
//                    2 group, 3 block) | drop mask << 27 (`drop_mask_names`) | block height << 30, or < 0
// batch key code: dtype code | kind << 4 | num_bits << 8, kind 0 int8, 1 fp8, 2 fp8 with float8 zero points, 3 int8 packed four to a word (w8_*)
// ------------------------------------------------------------------------------------------
inline int q8_code(at::ScalarType dt, int kind, int bits) { return half_code(dt) | (kind << 4) | (bits << 8); }

// codec.q8_batch_group: elements per scale, or 0.  strategy < 0: inferred from the scale's shape (forward.py:99-130)
int64_t q8_group(int64_t rows, int64_t cols, const at::Tensor& scale, const at::Tensor* zp, at::ScalarType wdt, const at::Device& dev, int strategy, int64_t group_size,
                 bool f8z, int64_t block_rows = 0) {
    if (!half_type(wdt) || scale.scalar_type() != wdt || scale.device() != dev || !scale.is_contiguous() || !aligned16(scale)) return 0;
    if (rows <= 0 || cols % 16) return 0;
    int64_t group = 0;
    if (scale.numel() == 1 && scale.dim() <= 1 && (strategy < 0 || strategy == 0)) group = rows * cols;
    else if (scale.dim() == 2 && scale.size(0) == rows && scale.size(1) == 1 && (strategy < 0 || strategy == 1)) group = cols;
    else if (scale.dim() == 2 && scale.size(0) == rows && scale.size(1) > 1 && cols % scale.size(1) == 0 && (strategy < 0 || strategy == 2)) {
        group = cols / scale.size(1);
        if (strategy == 2 && group_size && group_size != group) return 0;
    } else if (scale.dim() == 2 && (strategy < 0 || strategy == 3) && scale.size(0) >= 1 && scale.size(1) >= 1) {
        // block strategy: the table's group is -((rows per block << 24) | columns per block) (include/ct_hip.h)
        int64_t bh = block_rows, bw = group_size;
        if (strategy < 0) {
            if (rows % scale.size(0) || cols % scale.size(1)) return 0;
            bh = rows / scale.size(0);
            bw = cols / scale.size(1);
        }
        if (bh < 1 || bw < 16 || (bh & (bh - 1)) || (bw & (bw - 1)) || bh >= (int64_t(1) << 24) || bw >= (int64_t(1) << 24) || cols % bw ||
            rows * cols >= (int64_t(1) << 34) || scale.size(0) != (rows + bh - 1) / bh || scale.size(1) != cols / bw)
            return 0;
        group = -((bh << 24) | bw);
    } else return 0;
    if (group > 0 && group % 16) return 0;
    if (zp && (zp->scalar_type() != (f8z ? at::kFloat8_e4m3fn : at::kChar) || zp->sizes() != scale.sizes() || zp->device() != dev || !zp->is_contiguous())) return 0;
    return group;
}

// the entries the 8-bit loops (q8, mx8, w8 compress) read the same way: a dense `weight`, a scale, a zero point or none, no activation ordering
struct Q8Entries {
    const at::Tensor *w, *scale, *zp;
    bool ok;
    explicit Q8Entries(const Entries& e) : w(e.tensor(N.weight)), scale(e.tensor(N.weight_scale)), zp(e.tensor(N.weight_zero_point)) {
        ok = w && scale && !e.has(N.weight_g_idx) && tensor_or_absent(e, zp, N.weight_zero_point) && dense_source(*w);
    }
};

bool q8_take_compress(PyObject* m, int64_t info, Entries& e, Sink& sink) {
    const int64_t group_size = info & 0xfffff, block_rows = (info >> 30) & 0xfffff;
    const int bits = (int)((info >> 20) & 15), strategy = (int)((info >> 25) & 3), dropmask = (int)((info >> 27) & 7);
    const bool is_float = ((info >> 24) & 1) != 0;
    if (info < 0) return false;
    const Q8Entries q(e);
    if (!(q.ok && bits >= 1 && bits <= 8 && (!is_float || bits == 8))) return false;
    const at::Tensor *w = q.w, *zp = q.zp;
    const bool f8z = is_float && zp && zp->scalar_type() == at::kFloat8_e4m3fn;
    if (is_float && zp && !f8z) return false;
    const int64_t rows = w->size(0), cols = w->size(1);
    const int64_t group = q8_group(rows, cols, *q.scale, zp, w->scalar_type(), w->device(), strategy, group_size, f8z, block_rows);
    if (group == 0 || !staying_entries_are_final(e, {N.weight}, dropmask)) return false;
    at::Tensor out = at::empty({rows, cols}, w->options().dtype(is_float ? at::kFloat8_e4m3fn : at::kChar));
    Batch& b = sink.at(*w, q8_code(w->scalar_type(), is_float ? (f8z ? 2 : 1) : 0, bits));
    b.row(item_row(w->data_ptr(), q.scale->data_ptr(), data_or_null(zp), out.data_ptr(), rows, cols, group));
    // (module, codes, drop mask, keep-alive weight, keep-alive zero point or None)
    b.jobs.append(py::make_tuple(borrowed(m), wrap(out), dropmask, entry_ref(e, N.weight), zp ? entry_ref(e, N.weight_zero_point) : py::none()));
    return true;
}

// the codes replace `weight` (re-added last, as swap_direct_entries with `weight` among the removed names), a symmetric scheme's zero points leave
void q8_finish(py::list jobs, py::object status) {
    finish_jobs(jobs, status.ptr(), [](PyObject* job, Entries& e) {
        drop_zero_points(e, PyLong_AsLong(PyTuple_GET_ITEM(job, 2)));
        drop(e.params, N.weight);  // `compress` / `decompress` pop `weight` and add the result last (naive_quantized/base.py:62-126): it ends up behind the entries that stay
        set_entry(e, N.weight, job_tensor(job, 1));
    });
}

// decompress infos[i]: > 0 when the module's codec is the plain 8-bit one (the layout is read off the stored tensors, as `dequantize` does), else 0
bool q8_take_decompress(PyObject* m, int64_t info, Entries& e, Sink& sink) {
    if (info <= 0) return false;
    const Q8Entries q(e);
    if (!q.ok) return false;
    const at::Tensor *codes = q.w, *scale = q.scale, *zp = q.zp;
    int kind = codes->scalar_type() == at::kChar ? 0 : codes->scalar_type() == at::kFloat8_e4m3fn ? 1 : -1;
    const bool f8z = kind == 1 && zp && zp->scalar_type() == at::kFloat8_e4m3fn;
    if (kind < 0 || (kind == 1 && zp && !f8z)) return false;
    if (f8z) kind = 2;
    const int64_t rows = codes->size(0), cols = codes->size(1);
    const int64_t group = q8_group(rows, cols, *scale, zp, scale->scalar_type(), codes->device(), -1, 0, f8z);
    if (group == 0 || !staying_entries_are_final(e, {N.weight})) return false;
    at::Tensor out = at::empty({rows, cols}, scale->options());
    Batch& b = sink.at(*codes, q8_code(scale->scalar_type(), kind, 8));
    b.row(item_row(codes->data_ptr(), scale->data_ptr(), data_or_null(zp), out.data_ptr(), rows, cols, group));
    b.jobs.append(py::make_tuple(borrowed(m), wrap(out), 0, entry_ref(e, N.weight), py::none()));  // q8_finish's job: nothing to drop
    return true;
}


// the quantized modules of a model in `named_modules(remove_duplicate=True)` order (pre-order over `_modules`, every module once):
// model_compressor.py:152-164,191-195 with is_module_quantized (quantization/utils/helpers.py:229-250: a scheme with at least one of
// weights / input_activations / output_activations).  300 modules cost the interpreter 0.3 ms per walk; here ~30 us.
// named_modules(remove_duplicate=True) order (pre-order, children in `_modules` order, a module reached twice is visited once), on an explicit
// stack; `take(n)` returns the next n quantized modules and keeps its place.  (Resumable because ModelCompressor once launched the first 32
// modules of a model before walking the rest; that measured slower — DESIGN.md 5.5 — and the one caller left takes everything.)
struct ModuleWalk {
    PyObject* modules_name = PyUnicode_InternFromString("_modules");
    PyObject* scheme_name = PyUnicode_InternFromString("quantization_scheme");
    PyObject* arg_names[3] = {PyUnicode_InternFromString("weights"), PyUnicode_InternFromString("input_activations"),
                              PyUnicode_InternFromString("output_activations")};
    std::unordered_set<PyObject*> seen;
    std::vector<std::pair<py::object, Py_ssize_t>> stack;  // (a module's `_modules` dictionary, position of its iteration)
    py::object root;  // until the first take

    explicit ModuleWalk(py::object model) : root(std::move(model)) {}

    void enter(PyObject* module, py::list& out) {
        if (!seen.insert(module).second) return;
        PyObject* scheme = lookup_plain(module, scheme_name);
        if (scheme) {
            bool quantized = false;
            if (scheme != Py_None) {
                for (PyObject* a : arg_names) {
                    PyObject* v = PyObject_GetAttr(scheme, a);
                    if (!v) {
                        PyErr_Clear();
                        continue;
                    }
                    quantized = quantized || v != Py_None;
                    Py_DECREF(v);
                }
            }
            Py_DECREF(scheme);
            if (quantized) out.append(py::reinterpret_borrow<py::object>(module));
        }
        PyObject* children = lookup_plain(module, modules_name);
        if (!children) return;
        if (PyDict_Check(children) && PyDict_Size(children) > 0) stack.emplace_back(py::reinterpret_steal<py::object>(children), 0);
        else Py_DECREF(children);
    }

    // the next `n` quantized modules (all that are left when n < 0)
    py::list take(Py_ssize_t n) {
        py::list out;
        if (root) {
            py::object r = std::move(root);
            root = py::object();
            enter(r.ptr(), out);
        }
        while (!stack.empty() && (n < 0 || PyList_GET_SIZE(out.ptr()) < n)) {
            PyObject *key, *value;
            const size_t top = stack.size() - 1;
            if (PyDict_Next(stack[top].first.ptr(), &stack[top].second, &key, &value)) {
                if (value != Py_None) enter(value, out);  // may push: `stack[top]` is not touched after this
            } else {
                stack.pop_back();
            }
        }
        return out;
    }

    bool done() const { return !root && stack.empty(); }
};

py::list quantized_modules(py::object model) {
    touch_tls();
    return ModuleWalk(std::move(model)).take(-1);
}

// ------------------------------------------------------------------------------------------
// The two plug-in calls that WAIT for the device before they return (include/ct_hip.h "Host mailbox"): the sparse-bitmask
// compress (nnz sizes `values`) and the default mode of the marlin-24 compress (the 2:4 verdict raises from the call).  Their
// kernels run 30-42 us at 8192^2; the interpreter's share of one call — four torch.empty, a twelve-argument ctypes call, the
// mailbox wait, the slice — was 15-20 us in FRONT of and behind that, serial with it by construction.  Here the same steps
// (allocate with ATen, launch through the C ABI, spin on the mailbox / the stream, narrow) run without the interpreter.  The C-ABI
// entries are reached through their addresses (bind_abi: taken from the ctypes handle of libct_hip.so, so this extension links
// nothing of HIP); a non-zero status is handed back for _lib.check to raise (ct_last_error is thread-local: same thread).
// ------------------------------------------------------------------------------------------
using bitmask_compress_fn = int (*)(const void*, int, int64_t, int64_t, void*, int64_t, uint8_t*, int64_t*, int64_t*, void*, int64_t, void*);
using workspace_bytes_fn = int64_t (*)(int64_t, int64_t);
using mailbox_wait_fn = int (*)(const int64_t*, int64_t, void*, int64_t*);
using stream_wait_fn = int (*)(void*);
using marlin_full_fn = int (*)(const void*, int, const void*, int, const void*, int, int64_t, int64_t, int64_t, int, int32_t*, int16_t*, void*, int*, int, void*);
using marlin_verdict_fn = int (*)(const void*, int, const void*, int, const void*, int, int64_t, int64_t, int64_t, int, int32_t*, int16_t*, void*, int64_t*, void*, int, void*);

struct Abi {
    bitmask_compress_fn bitmask_compress = nullptr;
    workspace_bytes_fn bitmask_workspace_bytes = nullptr;
    mailbox_wait_fn mailbox_wait = nullptr;
    stream_wait_fn stream_wait = nullptr;
    marlin_full_fn marlin_full = nullptr;
    marlin_verdict_fn marlin_verdict = nullptr;  // optional (an older libct_hip.so): the full entry + a stream wait then
    stream_wait_fn hip_stream_synchronize = nullptr;  // optional: hipStreamSynchronize of the HIP runtime that is already loaded
    // the batched sparse-bitmask compress (round 6): plan + launch of the table kernel, and the batched copy that makes the results exact-size
    int64_t (*bitmask_batch_plan)(void*, int, int64_t*) = nullptr;
    int (*bitmask_compress_batch)(const void*, int, int64_t, int, void*, int64_t, void*) = nullptr;
    int64_t (*copy_batch_plan)(void*, int) = nullptr;
    int (*copy_batch)(const void*, int, int64_t, void*) = nullptr;
    int64_t (*bitmask_decompress_batch_plan)(void*, int) = nullptr;
    int (*bitmask_decompress_batch)(const void*, int, int64_t, int, void*) = nullptr;
} g_abi;

// 1: the waits below as described there; 0: only through ct_mailbox_wait_i64 / ct_stream_wait (tools/exp_r04.py compares the two on one lease)
int g_wait_mode = 1;

// the word a kernel stores into pinned host memory, as soon as it differs from `pending`: plain reads of the (cached, coherent) word with a pause
// between them — ct_mailbox_wait_i64 looks at the stream every 64 reads, and a hipStreamQuery is 1-2 us during which the word is not looked at.  After
// ~1 ms without the word (a failed launch, a kernel that does not write it) the C-ABI wait takes over, with its stream check and its error reporting.
inline bool spin_for_word(const volatile int64_t* word, int64_t pending, int64_t* value) {
    for (unsigned spin = 0; spin < (1u << 18); ++spin) {
        const int64_t v = *word;
        if (v != pending) {
            *value = v;
            return true;
        }
        __builtin_ia32_pause();
    }
    return false;
}

void bind_abi(const std::map<std::string, uintptr_t>& addr) {
    auto at = [&](const char* name) {
        auto it = addr.find(name);
        if (it == addr.end() || !it->second) throw std::runtime_error(std::string("bind_abi: no address for ") + name);
        return it->second;
    };
    g_abi.bitmask_compress = reinterpret_cast<bitmask_compress_fn>(at("ct_bitmask_compress"));
    g_abi.bitmask_workspace_bytes = reinterpret_cast<workspace_bytes_fn>(at("ct_bitmask_compress_workspace_bytes"));
    g_abi.mailbox_wait = reinterpret_cast<mailbox_wait_fn>(at("ct_mailbox_wait_i64"));
    g_abi.stream_wait = reinterpret_cast<stream_wait_fn>(at("ct_stream_wait"));
    g_abi.marlin_full = reinterpret_cast<marlin_full_fn>(at("ct_marlin24_compress_w4_full"));
    auto mv = addr.find("ct_marlin24_compress_w4_verdict");
    g_abi.marlin_verdict = mv != addr.end() && mv->second ? reinterpret_cast<marlin_verdict_fn>(mv->second) : nullptr;
    auto opt = addr.find("hipStreamSynchronize");
    g_abi.hip_stream_synchronize = opt != addr.end() && opt->second ? reinterpret_cast<stream_wait_fn>(opt->second) : nullptr;
    auto find = [&](const char* name) -> uintptr_t {
        auto it = addr.find(name);
        return it != addr.end() ? it->second : 0;
    };
    g_abi.bitmask_batch_plan = reinterpret_cast<int64_t (*)(void*, int, int64_t*)>(find("ct_bitmask_batch_plan"));
    g_abi.bitmask_compress_batch = reinterpret_cast<int (*)(const void*, int, int64_t, int, void*, int64_t, void*)>(find("ct_bitmask_compress_batch"));
    g_abi.copy_batch_plan = reinterpret_cast<int64_t (*)(void*, int)>(find("ct_copy_batch_plan"));
    g_abi.copy_batch = reinterpret_cast<int (*)(const void*, int, int64_t, void*)>(find("ct_copy_batch"));
    g_abi.bitmask_decompress_batch_plan = reinterpret_cast<int64_t (*)(void*, int)>(find("ct_bitmask_decompress_batch_plan"));
    g_abi.bitmask_decompress_batch = reinterpret_cast<int (*)(const void*, int, int64_t, int, void*)>(find("ct_bitmask_decompress_batch"));
}

bool on_device(const at::Tensor& t) { return t.is_cuda() || (g_allow_cpu && t.is_cpu()); }

// codec.bitmask_compress for a contiguous, 16-byte aligned device tensor whose device is the current one (the caller checks the
// last; everything else is checked here and answered with None: the Python path takes the call).  `dt`: the C ABI's element code.
// Returns (status, values, bitmask, row_offsets).
// `exact`: `values` owns exactly nnz elements (the kept prefix is copied out of the worst-case buffer, which goes back to the allocator); else a view of it.
py::object bitmask_compress(const at::Tensor& x, int dt, uintptr_t mailbox_host, uintptr_t mailbox_dev, uintptr_t stream, bool exact) {
    touch_tls();
    if (!g_abi.bitmask_compress || !on_device(x) || x.dim() < 1 || !x.is_contiguous() || (reinterpret_cast<uintptr_t>(x.data_ptr()) & 15) || x.numel() == 0)
        return py::none();
    const int64_t cols = x.size(-1), numel = x.numel(), rows = numel / cols;
    const int64_t ws_bytes = g_abi.bitmask_workspace_bytes(rows, cols);
    const auto opts = x.options();
    at::Tensor bitmask = at::empty({rows, (cols + 7) / 8}, opts.dtype(at::kByte));
    at::Tensor row_offsets = at::empty({rows}, opts.dtype(at::kLong));
    at::Tensor workspace = at::empty({ws_bytes / 8 + 1}, opts.dtype(at::kLong));
    at::Tensor buf = at::empty({numel}, opts);
    int status;
    int64_t nnz = -1;
    {
        py::gil_scoped_release nogil;  // as the ctypes calls this replaces: other threads run while this one spins
        volatile int64_t* word = reinterpret_cast<volatile int64_t*>(mailbox_host);
        *word = -1;
        status = g_abi.bitmask_compress(x.data_ptr(), dt, rows, cols, buf.data_ptr(), numel, bitmask.data_ptr<uint8_t>(), row_offsets.data_ptr<int64_t>(),
                                        reinterpret_cast<int64_t*>(mailbox_dev), workspace.data_ptr(), ws_bytes, reinterpret_cast<void*>(stream));
        if (status == 0 && !(g_wait_mode && spin_for_word(word, -1, &nnz)))
            status = g_abi.mailbox_wait(reinterpret_cast<const int64_t*>(mailbox_host), -1, reinterpret_cast<void*>(stream), &nnz);
    }
    if (status != 0) return py::make_tuple(status, py::none(), py::none(), py::none());
    if (nnz < 0 || nnz > numel) throw std::runtime_error("bitmask_compress: the device reported an impossible number of kept values");
    // codec.bitmask_compress: same rule
    at::Tensor values = buf.narrow(0, 0, nnz);
    if (exact && nnz != numel) values = values.clone();
    return py::make_tuple(0, values, bitmask, row_offsets);
}

// codec.bitmask_compress_many (round 6): a LIST of tensors — a checkpoint's sparse weights — in ONE kernel launch per window.
// A single ct_bitmask_compress launch of a checkpoint-sized tensor is a latency chain (9 us for 1 MB, 10 us for 8 MB: 2-16 % of the HBM rate)
// and the call around it waits ~9 us more for nnz; here a window of tensors goes into one table (ct_bitmask_compress_batch: the chains run side
// by side), each tensor reports its nnz into its own word of the thread's mailbox, and the host reads the words when the launch is under way:
// one launch and one wait per window.  `exact`: the kernel writes into ONE worst-case arena and every `values` is an exact-size allocation
// filled by ONE batched copy (ct_copy_batch); otherwise every tensor gets its own worst-case buffer and `values` is a view of it.
// A window ends after `nwords` tensors, `arena_budget` bytes of worst-case space (never less than one tensor), or a change of element size
// (a table holds ONE element size).  `dts[i]` < 0, rows that are not whole 16-byte units and whatever the single-tensor path would decline -> None at that position
// (the Python caller takes those one by one).
at::Tensor upload_words(const std::vector<int64_t>& v, const at::TensorOptions& dev_opts) {
    // pinned staging: the copy is asynchronous and the caching host allocator recycles the block only when the copy has completed
    at::Tensor host = dev_opts.device().is_cuda() ? at::empty({(int64_t)v.size()}, at::TensorOptions().dtype(at::kLong).pinned_memory(true))
                                                  : at::empty({(int64_t)v.size()}, at::TensorOptions().dtype(at::kLong));
    std::memcpy(host.data_ptr(), v.data(), v.size() * sizeof(int64_t));
    return dev_opts.device().is_cuda() ? host.to(dev_opts.device(), /*non_blocking=*/true) : host;
}

py::list bitmask_compress_many(const std::vector<at::Tensor>& xs, const std::vector<int>& dts, uintptr_t mailbox_host, uintptr_t mailbox_dev, int word0, int nwords,
                               uintptr_t stream, bool exact, int64_t arena_budget) {
    touch_tls();
    if (!g_abi.bitmask_batch_plan || !g_abi.bitmask_compress_batch || !g_abi.copy_batch_plan || !g_abi.copy_batch)
        throw std::runtime_error("bitmask_compress_many: bind_abi has not bound the batch entries");
    if (xs.size() != dts.size() || nwords < 2) throw std::runtime_error("bitmask_compress_many: bad arguments");
    const size_t n = xs.size();
    std::vector<py::object> results(n, py::none());
    struct Slot {
        size_t index;
        int64_t rows, cols, numel, offset;
        at::Tensor bitmask, row_offsets, buf;
    };
    // TWO windows in flight: while the device works on window k the host plans and launches window k + 1, and only then reads window k's words —
    // the mailbox words are split into two halves that the windows take in turn
    struct Window {
        std::vector<Slot> slots;
        at::Tensor arena, table_dev, workspace;
        int word_base = 0;
        int64_t es = 2;
    };
    const int half = nwords / 2;
    auto pad = [](int64_t b) { return (b + 255) / 256 * 256; };
    auto eligible = [&](size_t i) {
        const at::Tensor& x = xs[i];
        const int64_t es = (int64_t)x.element_size();
        return dts[i] >= 0 && (es == 1 || es == 2 || es == 4) && on_device(x) && x.dim() >= 1 && x.is_contiguous() &&
               (reinterpret_cast<uintptr_t>(x.data_ptr()) & 15) == 0 && x.numel() > 0 && (x.size(-1) * es) % 16 == 0 && x.numel() * es <= (int64_t(1) << 30);
    };
    auto fail = [](int status) {
        py::list out;
        out.append(py::int_(status));
        return out;
    };

    // plan + launch: allocations, the table, ONE kernel launch; nothing is waited for
    auto launch = [&](Window& w) -> int {
        const auto opts = xs[w.slots[0].index].options();
        int64_t arena_bytes = 0;
        for (auto& sl : w.slots) arena_bytes = sl.offset + pad(sl.numel * w.es);
        if (exact) w.arena = at::empty({arena_bytes}, opts.dtype(at::kByte));
        volatile int64_t* words = reinterpret_cast<volatile int64_t*>(mailbox_host) + w.word_base;
        std::vector<int64_t> table;
        table.reserve(w.slots.size() * 15);
        for (size_t k = 0; k < w.slots.size(); ++k) {
            Slot& sl = w.slots[k];
            const at::Tensor& x = xs[sl.index];
            sl.bitmask = at::empty({sl.rows, (sl.cols + 7) / 8}, opts.dtype(at::kByte));
            sl.row_offsets = at::empty({sl.rows}, opts.dtype(at::kLong));
            void* values_ptr;
            if (exact) {
                values_ptr = static_cast<uint8_t*>(w.arena.data_ptr()) + sl.offset;
            } else {
                sl.buf = at::empty({sl.numel}, x.options());
                values_ptr = sl.buf.data_ptr();
            }
            words[k] = -1;
            // struct ct_bitmask_item (include/ct_hip.h): x, values, bitmask, row_offsets, total, rows, cols, values_capacity, {dt, is_float}, then 6 derived words
            const int64_t row[15] = {(int64_t)(uintptr_t)x.data_ptr(), (int64_t)(uintptr_t)values_ptr, (int64_t)(uintptr_t)sl.bitmask.data_ptr(),
                                     (int64_t)(uintptr_t)sl.row_offsets.data_ptr(), (int64_t)(mailbox_dev + 8 * (uintptr_t)(w.word_base + (int)k)), sl.rows, sl.cols, sl.numel,
                                     (int64_t)(uint32_t)dts[sl.index], 0, 0, 0, 0, 0, 0};
            table.insert(table.end(), row, row + 15);
        }
        int64_t ws_bytes = 0;
        const int64_t blocks = g_abi.bitmask_batch_plan(table.data(), (int)w.slots.size(), &ws_bytes);
        if (blocks < 0) return 1;  // CT_ERR_INVALID_ARG: ct_last_error has the text
        w.table_dev = upload_words(table, opts);
        w.workspace = at::empty({ws_bytes / 8 + 1}, opts.dtype(at::kLong));
        return g_abi.bitmask_compress_batch(w.table_dev.data_ptr(), (int)w.slots.size(), blocks, (int)w.es, w.workspace.data_ptr(), ws_bytes, reinterpret_cast<void*>(stream));
    };

    // the window's nnz words, the exact-size results (one batched copy), the tuples
    auto finish = [&](Window& w) -> int {
        const auto opts = xs[w.slots[0].index].options();
        volatile int64_t* words = reinterpret_cast<volatile int64_t*>(mailbox_host) + w.word_base;
        std::vector<int64_t> nnz(w.slots.size(), -1);
        int status = 0;
        {
            py::gil_scoped_release nogil;
            for (size_t k = 0; k < w.slots.size() && status == 0; ++k)
                if (!(g_wait_mode && spin_for_word(words + k, -1, &nnz[k])))
                    status = g_abi.mailbox_wait(reinterpret_cast<const int64_t*>(mailbox_host) + w.word_base + k, -1, reinterpret_cast<void*>(stream), &nnz[k]);
        }
        if (status != 0) return status;
        std::vector<int64_t> copies;
        std::vector<at::Tensor> values(w.slots.size());
        for (size_t k = 0; k < w.slots.size(); ++k) {
            Slot& sl = w.slots[k];
            const at::Tensor& x = xs[sl.index];
            if (nnz[k] < 0 || nnz[k] > sl.numel) throw std::runtime_error("bitmask_compress_many: the device reported an impossible number of kept values");
            if (exact) {
                values[k] = at::empty({nnz[k]}, x.options());  // exact size; the arena goes back when the window is done
                const int64_t item[4] = {(int64_t)(uintptr_t)(static_cast<uint8_t*>(w.arena.data_ptr()) + sl.offset), (int64_t)(uintptr_t)values[k].data_ptr(), nnz[k] * w.es, 0};
                copies.insert(copies.end(), item, item + 4);
            } else {
                values[k] = sl.buf.narrow(0, 0, nnz[k]);
            }
        }
        if (exact) {
            const int64_t cblocks = g_abi.copy_batch_plan(copies.data(), (int)w.slots.size());
            if (cblocks < 0) return 1;
            if (cblocks > 0) {
                at::Tensor copies_dev = upload_words(copies, opts);
                status = g_abi.copy_batch(copies_dev.data_ptr(), (int)w.slots.size(), cblocks, reinterpret_cast<void*>(stream));
                if (status != 0) return status;
            }
        }
        for (size_t k = 0; k < w.slots.size(); ++k) results[w.slots[k].index] = py::make_tuple(values[k], w.slots[k].bitmask, w.slots[k].row_offsets);
        return 0;
    };

    std::vector<bool> taken(n, false);
    std::unique_ptr<Window> pending;  // launched, not yet finished
    int turn = 0;
    for (size_t start = 0; start < n; ++start) {
        if (taken[start] || !eligible(start)) continue;
        // a window: the next eligible tensors of this one's device and element size, as many as half the words / the arena budget allow
        std::unique_ptr<Window> w(new Window);
        w->es = (int64_t)xs[start].element_size();
        w->word_base = word0 + (turn & 1) * half;
        int64_t arena_bytes = 0;
        for (size_t i = start; i < n && (int)w->slots.size() < half; ++i) {
            if (taken[i] || !eligible(i) || (int64_t)xs[i].element_size() != w->es || xs[i].device() != xs[start].device()) continue;
            const int64_t bytes = pad(xs[i].numel() * w->es);
            if (!w->slots.empty() && arena_bytes + bytes > arena_budget) break;
            Slot sl;
            sl.index = i;
            sl.cols = xs[i].size(-1);
            sl.numel = xs[i].numel();
            sl.rows = sl.numel / sl.cols;
            sl.offset = arena_bytes;
            arena_bytes += bytes;
            w->slots.push_back(std::move(sl));
            taken[i] = true;
        }
        int status = launch(*w);
        if (status == 0 && pending) status = finish(*pending);  // the previous window, while this one runs
        if (status != 0) return fail(status);  // reported the C ABI's way by the caller (_lib.check: ct_last_error is this thread's)
        pending = std::move(w);
        ++turn;
    }
    if (pending) {
        const int status = finish(*pending);
        if (status != 0) return fail(status);
    }
    py::list out;
    out.append(py::int_(0));
    for (auto& r : results) out.append(r);
    return out;
}

// codec.bitmask_decompress_many (round 6): loading a sparse checkpoint — a LIST of (values, bitmask, row_offsets, shape) — in ONE launch per
// element size (ct_bitmask_decompress_batch): the dense outputs are allocated here, the table is planned and uploaded, nothing is waited for.
// `dts[i]` < 0 and whatever the table kernel does not take (8-bit payloads, rows that are not whole 64-byte runs, a missing row_offsets, another
// device, views) -> None at that position: the Python caller decompresses those one by one.  Returns [status, result or None, ...].
py::list bitmask_decompress_many(const std::vector<at::Tensor>& values, const std::vector<at::Tensor>& bitmasks, const std::vector<c10::optional<at::Tensor>>& row_offsets,
                                 const std::vector<std::vector<int64_t>>& shapes, const std::vector<int>& dts, uintptr_t stream) {
    touch_tls();
    if (!g_abi.bitmask_decompress_batch_plan || !g_abi.bitmask_decompress_batch) throw std::runtime_error("bitmask_decompress_many: bind_abi has not bound the batch entries");
    const size_t n = values.size();
    if (bitmasks.size() != n || row_offsets.size() != n || shapes.size() != n || dts.size() != n) throw std::runtime_error("bitmask_decompress_many: bad arguments");
    std::vector<py::object> results(n, py::none());
    auto eligible = [&](size_t i, int64_t& rows, int64_t& cols) {
        const at::Tensor &v = values[i], &b = bitmasks[i];
        const int64_t es = (int64_t)v.element_size();
        if (dts[i] < 0 || (es != 2 && es != 4) || shapes[i].empty() || !row_offsets[i].has_value()) return false;
        cols = shapes[i].back();
        rows = 1;
        for (size_t k = 0; k + 1 < shapes[i].size(); ++k) rows *= shapes[i][k];
        const at::Tensor& ro = *row_offsets[i];
        return rows > 0 && cols > 0 && (cols * es) % 64 == 0 && on_device(v) && on_device(b) && on_device(ro) && v.device() == b.device() && ro.device() == b.device() &&
               v.is_contiguous() && b.is_contiguous() && ro.is_contiguous() && v.dim() == 1 && b.scalar_type() == at::kByte && b.numel() == rows * ((cols + 7) / 8) &&
               ro.scalar_type() == at::kLong && ro.numel() == rows && (reinterpret_cast<uintptr_t>(v.data_ptr()) & 15) == 0 && (reinterpret_cast<uintptr_t>(b.data_ptr()) & 3) == 0;
    };
    std::vector<bool> taken(n, false);
    for (size_t start = 0; start < n; ++start) {
        int64_t rows = 0, cols = 0;
        if (taken[start] || !eligible(start, rows, cols)) continue;
        const int64_t es = (int64_t)values[start].element_size();
        const auto dev = bitmasks[start].device();
        std::vector<int64_t> table;
        std::vector<size_t> index;
        std::vector<at::Tensor> outs;
        for (size_t i = start; i < n; ++i) {
            if (taken[i] || !eligible(i, rows, cols) || (int64_t)values[i].element_size() != es || bitmasks[i].device() != dev) continue;
            taken[i] = true;
            at::Tensor out = at::empty(shapes[i], values[i].options());
            // struct ct_bitmask_ditem: values, bitmask, row_offsets, out, rows, cols, values_len, {dt, single}, first_block
            const int64_t row[9] = {(int64_t)(uintptr_t)values[i].data_ptr(), (int64_t)(uintptr_t)bitmasks[i].data_ptr(), (int64_t)(uintptr_t)row_offsets[i]->data_ptr(),
                                    (int64_t)(uintptr_t)out.data_ptr(), rows, cols, values[i].numel(), (int64_t)(uint32_t)dts[i], 0};
            table.insert(table.end(), row, row + 9);
            index.push_back(i);
            outs.push_back(std::move(out));
        }
        const int64_t blocks = g_abi.bitmask_decompress_batch_plan(table.data(), (int)index.size());
        int status = blocks < 0 ? 1 : 0;
        if (status == 0 && blocks > 0) {
            at::Tensor table_dev = upload_words(table, values[start].options());
            status = g_abi.bitmask_decompress_batch(table_dev.data_ptr(), (int)index.size(), blocks, (int)es, reinterpret_cast<void*>(stream));
        }
        if (status != 0) {
            py::list out;
            out.append(py::int_(status));
            return out;
        }
        for (size_t k = 0; k < index.size(); ++k) results[index[k]] = py::reinterpret_steal<py::object>(THPVariable_Wrap(outs[k]));
    }
    py::list out;
    out.append(py::int_(0));
    for (auto& r : results) out.append(r);
    return out;
}

// the default (raise-from-the-call) mode of Marlin24Compressor.compress for int4: ct_marlin24_compress_w4_full, then a spin on the stream,
// then the verdict word.  The caller has validated shapes / dtypes / contiguity (compressors/sparse/marlin_24.py).  Returns
// (status, violated, weight_packed, meta, scale_packed).
// `verdict_ws`: the caller's ticket tree for the verdict entry (include/ct_hip.h: CT_M24_VERDICT_WORKSPACE_BYTES of zeroed device memory, one per
// (thread, device) next to the mailbox — _lib.Mailbox.verdict_workspace); 0: the full entry + a stream wait.
py::tuple marlin24_w4_full(const at::Tensor& weight, int wdt, const at::Tensor& scale, int sdt, const c10::optional<at::Tensor>& zp, int zdt, int64_t group,
                           bool group_perm, uintptr_t flag_host, uintptr_t flag_dev, uintptr_t verdict_ws, uintptr_t stream) {
    if (!g_abi.marlin_full) throw std::runtime_error("marlin24_w4_full: bind_abi has not run");
    const int64_t m = weight.size(0), k = weight.size(1);
    const auto opts = weight.options();
    at::Tensor packed = at::empty({k / 32, m * 2}, opts.dtype(at::kInt));
    at::Tensor meta = at::empty({k / 32, m * 2}, opts.dtype(at::kShort));  // the (m, k/16) reordered matrix, viewed as upstream stores it
    at::Tensor scale_packed = at::empty({k / group, m}, opts.dtype(at::kHalf));
    int status;
    int64_t verdict = 0;
    bool violated = false;
    {
        py::gil_scoped_release nogil;
        volatile int64_t* word = reinterpret_cast<volatile int64_t*>(flag_host);
        *word = 0;
        const void* zptr = zp.has_value() ? zp->data_ptr() : nullptr;
        // Round 5: the launch's last-reporting workgroup stores the verdict (1 = 2:4 holds, 3 = violated) into the pinned word as soon as every
        // workgroup has evaluated its tiles — the host spins on the word as bitmask_compress does for nnz, instead of waiting for the stream to
        // drain (hipStreamSynchronize: +15 us over the kernel on the class call).  The outputs follow in stream order.
        status = -1;
        if (g_wait_mode && g_abi.marlin_verdict && verdict_ws) {
            status = g_abi.marlin_verdict(weight.data_ptr(), wdt, scale.data_ptr(), sdt, zptr, zp.has_value() ? zdt : -1, m, k, group, group_perm ? 1 : 0,
                                          packed.data_ptr<int32_t>(), meta.data_ptr<int16_t>(), scale_packed.data_ptr(), reinterpret_cast<int64_t*>(flag_dev),
                                          reinterpret_cast<void*>(verdict_ws), 0, reinterpret_cast<void*>(stream));
            if (status == 0) {
                if (!spin_for_word(word, 0, &verdict))  // ~1 ms without a verdict: the stream's own completion (and its error, if any)
                    status = g_abi.mailbox_wait(reinterpret_cast<const int64_t*>(flag_host), 0, reinterpret_cast<void*>(stream), &verdict);
                if (status == 0 && verdict != 1 && verdict != 3) throw std::runtime_error("marlin24_w4_full: the launch finished without a 2:4 verdict");
                violated = verdict == 3;
            }
        }
        if (status == -1 || status == 2 /* CT_ERR_UNSUPPORTED: not the one-launch layout */) {
            *word = 0;
            status = g_abi.marlin_full(weight.data_ptr(), wdt, scale.data_ptr(), sdt, zptr, zp.has_value() ? zdt : -1, m, k, group, group_perm ? 1 : 0,
                                       packed.data_ptr<int32_t>(), meta.data_ptr<int16_t>(), scale_packed.data_ptr(), reinterpret_cast<int*>(flag_dev), 0,
                                       reinterpret_cast<void*>(stream));
            // the flag is final only when the whole launch has completed.  hipStreamSynchronize waits on the queue's completion signal itself; a
            // spin on hipStreamQuery (ct_stream_wait) sees it 3-4 us later (`profiles/r04_host_wait_forms.json`: 22.2 vs 17.8 us around a tiny kernel).
            // An error from it is re-asked through ct_stream_wait, which reports it the C ABI's way.
            if (status == 0 && !(g_wait_mode && g_abi.hip_stream_synchronize && g_abi.hip_stream_synchronize(reinterpret_cast<void*>(stream)) == 0))
                status = g_abi.stream_wait(reinterpret_cast<void*>(stream));
            violated = *word != 0;
        }
    }
    return py::make_tuple(status, violated, packed, meta, scale_packed);
}


// pack-quantized with the other word widths (2 / 3 / 5 / 6 / 7 bits) and, for EVERY width, modules with activation ordering (a `weight_g_idx` entry; symmetric
// weights-only group / channel schemes): no table form exists for them, so this loop launches `ct_quant_pack` / `ct_unpack_dequant` per module BY ADDRESS on `stream` of device `device_index` (which the caller has
// made current) and rewrites the dictionary right behind each launch — the interpreter's 22-33 us per module become ~7.  Entries as the W4 loop leaves them.
// The loop head and the hand-back are `each_plain_module`'s; there is no table, so no plan driver and no finish.  A refused launch hands the module back too:
// the Python path repeats it and reports the library's message.
// infos[i]: group_size | ASYMMETRIC << 24 (the scheme stores its zero points packed along rows, pack_quantized/base.py:107-110: one more launch,
// ct_pack_int32_dim0 / ct_unpack_int32_dim0) | strategy << 25 (1 channel, 2 group) | num_bits << 28, or < 0.
using quant_pack_fn = int (*)(const void*, int, const void*, int, const void*, int, int64_t, int64_t, int64_t, int64_t, int64_t, const int32_t*, int, int, int32_t*, void*);
using unpack_dequant_fn = int (*)(const int32_t*, int64_t, int64_t, int64_t, int, const void*, int, const void*, int, int64_t, int64_t, int64_t, const int32_t*, void*, int, void*);
using gidx_fn = int (*)(const int32_t*, int64_t, int64_t, int32_t*, int32_t*, void*);
quant_pack_fn g_quant_pack = nullptr;
unpack_dequant_fn g_unpack_dequant = nullptr;
gidx_fn g_gidx_col_group = nullptr;  // optional: without it modules with activation ordering go back to the Python loop

using pack_dim0_fn = int (*)(const int8_t*, int64_t, int64_t, int, int32_t*, void*);
using unpack_dim0_fn = int (*)(const int32_t*, int64_t, int64_t, int64_t, int, int8_t*, void*);
pack_dim0_fn g_pack_dim0 = nullptr;      // optional: without them asymmetric schemes go back to the Python loop
unpack_dim0_fn g_unpack_dim0 = nullptr;

void bind_pack(uintptr_t quant_pack, uintptr_t unpack_dequant, uintptr_t gidx_col_group, uintptr_t pack_dim0, uintptr_t unpack_dim0) {
    g_quant_pack = reinterpret_cast<quant_pack_fn>(quant_pack);
    g_unpack_dequant = reinterpret_cast<unpack_dequant_fn>(unpack_dequant);
    g_gidx_col_group = reinterpret_cast<gidx_fn>(gidx_col_group);
    g_pack_dim0 = reinterpret_cast<pack_dim0_fn>(pack_dim0);
    g_unpack_dim0 = reinterpret_cast<unpack_dim0_fn>(unpack_dim0);
}

// the `col_group` table of a module with activation ordering (codec._col_group_of's device form: ct_gidx_col_group); cols + 1 words, the last one the
// kernels' scratch.  An undefined tensor: g_idx is not the plain case (int32, one entry per column, contiguous, on the weights' device).
at::Tensor col_group_of(const at::Tensor& g_idx, const at::Tensor& like, int64_t cols, int64_t group, uintptr_t stream) {
    if (!g_gidx_col_group || g_idx.scalar_type() != at::kInt || g_idx.numel() != cols || !g_idx.is_contiguous() || g_idx.device() != like.device()) return at::Tensor();
    at::Tensor cg = at::empty({cols + 1}, g_idx.options());
    if (g_idx.is_cuda() &&
        g_gidx_col_group(static_cast<const int32_t*>(g_idx.data_ptr()), cols, group, static_cast<int32_t*>(cg.data_ptr()), static_cast<int32_t*>(cg.data_ptr()) + cols,
                         reinterpret_cast<void*>(stream)) != 0)
        return at::Tensor();
    return cg;
}

// which modules the per-module loop is for: every one with activation ordering, and without it the widths that have no table (4 and — symmetric — 8 ride theirs)
inline bool wb_is_mine(const Entries& e, const at::Tensor* gidx, int bits, bool asym) {
    return gidx != nullptr || (!e.has(N.weight_g_idx) && bits != 4 && (bits != 8 || asym));
}

py::list wb_compress_modules(py::list modules, py::object infos_arg, int device_index, uintptr_t stream, py::object status) {
    if (!g_quant_pack) throw std::runtime_error("wb_compress_modules: bind_pack has not been called");
    return each_plain_module(modules, infos_arg.ptr(), [&](PyObject* m, int64_t info, Entries& e) {
        const int bits = (int)((info >> 28) & 15), strategy = (int)((info >> 25) & 3);
        const bool asym = ((info >> 24) & 1) != 0;
        if (!(info >= 0 && bits >= 1 && bits <= 8) || dict_has(m, N.weight_packed) || dict_has(m, N.weight_shape)) return false;
        const at::Tensor *w = e.tensor(N.weight), *scale = e.tensor(N.weight_scale), *zp = e.tensor(N.weight_zero_point), *gidx = e.tensor(N.weight_g_idx);
        // (scales and zero points need no alignment here, unlike the W4 table: ct_quant_pack reads them by element)
        if (!(w && scale && wb_is_mine(e, gidx, bits, asym) && tensor_or_absent(e, zp, N.weight_zero_point) && (!asym || (zp != nullptr && g_pack_dim0 != nullptr)) &&
              !e.has(N.weight_packed) && dense_source(*w, 16, device_index) && half_type(w->scalar_type()) && scale->scalar_type() == w->scalar_type() &&
              scale->device() == w->device() && scale->is_contiguous() && scale->dim() == 2 && (gidx == nullptr || strategy == 2)))
            return false;
        const int64_t rows = w->size(0), cols = w->size(1), group = strategy == 1 ? cols : (info & 0xfffff);
        if (!(rows > 0 && cols > 0 && group > 0 && cols % group == 0 && scale->size(0) == rows && scale->size(1) == cols / group)) return false;
        if (zp && !(zp->scalar_type() == at::kChar && zp->sizes() == scale->sizes() && zp->is_contiguous() && zp->device() == w->device())) return false;
        if (!staying_entries_are_final(e, {N.weight, N.weight_zero_point})) return false;
        at::Tensor cg;
        if (gidx) {
            cg = col_group_of(*gidx, *w, cols, group, stream);
            if (!cg.defined()) return false;
        }
        at::Tensor packed = at::empty({rows, (cols * bits + 31) / 32}, w->options().dtype(at::kInt));
        const int dt = half_code(w->scalar_type());
        if (!w->is_cpu() && g_quant_pack(w->data_ptr(), dt, scale->data_ptr(), dt, data_or_null(zp), zp ? CT_I8 : -1, rows, cols, 1, group, cols / group,
                                         cg.defined() ? static_cast<const int32_t*>(cg.data_ptr()) : nullptr, bits, dt, static_cast<int32_t*>(packed.data_ptr()),
                                         reinterpret_cast<void*>(stream)) != 0)
            return false;
        at::Tensor zpp;
        if (asym) {  // pack_to_int32(zp, num_bits, packed_dim=0)
            zpp = at::empty({(rows * bits + 31) / 32, zp->size(1)}, w->options().dtype(at::kInt));
            if (!w->is_cpu() && g_pack_dim0(static_cast<const int8_t*>(zp->data_ptr()), rows, zp->size(1), bits, static_cast<int32_t*>(zpp.data_ptr()), reinterpret_cast<void*>(stream)) != 0)
                return false;
        }
        drop(e.params, N.weight);
        if (asym) set_entry(e, N.weight_zero_point, zpp);  // in place: same position
        else drop(e.params, N.weight_zero_point);  // a symmetric scheme stores none (compressors/base.py: symmetric_zp_keys)
        set_entry(e, N.weight_packed, packed);
        set_entry(e, N.weight_shape, shape_tensor(rows, cols));
        set_status(m, status.ptr());
        return true;
    });
}

py::list wb_decompress_modules(py::list modules, py::object infos_arg, int device_index, uintptr_t stream, py::object status) {
    if (!g_unpack_dequant) throw std::runtime_error("wb_decompress_modules: bind_pack has not been called");
    return each_plain_module(modules, infos_arg.ptr(), [&](PyObject* m, int64_t info, Entries& e) {
        const int bits = (int)((info >> 28) & 15);
        const bool asym = ((info >> 24) & 1) != 0;
        if (!(info >= 0 && bits >= 1 && bits <= 8) || dict_has(m, N.weight)) return false;
        const at::Tensor *packed = e.tensor(N.weight_packed), *scale = e.tensor(N.weight_scale), *gidx = e.tensor(N.weight_g_idx), *zpp = e.tensor(N.weight_zero_point);
        int64_t rows = 0, cols = 0;
        if (!(packed && scale && wb_is_mine(e, gidx, bits, asym) && (asym ? (zpp != nullptr && g_unpack_dim0 != nullptr) : !e.has(N.weight_zero_point)) && !e.has(N.weight) &&
              dense_source(*packed, 16, device_index) && packed->scalar_type() == at::kInt && scale->dim() == 2 && half_type(scale->scalar_type()) && scale->is_contiguous() &&
              scale->device() == packed->device() && stored_shape(e.tensor(N.weight_shape), rows, cols)))
            return false;
        // (R, 1): channel; (R, G): groups of cols / G — the layout upstream's argument-free dequantize infers (forward.py:99-130)
        if (!(scale->size(0) == rows && scale->size(1) > 0 && cols % scale->size(1) == 0 && packed->size(0) == rows && packed->size(1) == (cols * bits + 31) / 32 &&
              staying_entries_are_final(e, {N.weight_packed, N.weight_zero_point})))
            return false;
        const int64_t group = cols / scale->size(1);
        if (asym && !(zpp->scalar_type() == at::kInt && zpp->dim() == 2 && zpp->size(0) == (rows * bits + 31) / 32 && zpp->size(1) == scale->size(1) && zpp->is_contiguous() &&
                      zpp->device() == packed->device()))
            return false;
        at::Tensor cg;
        if (gidx) {
            cg = col_group_of(*gidx, *packed, cols, group, stream);
            if (!cg.defined()) return false;
        }
        at::Tensor out = at::empty({rows, cols}, scale->options());
        const int dt = half_code(scale->scalar_type());
        at::Tensor zp8;
        if (asym) {  // unpack_from_int32(zp, num_bits, (rows, G), packed_dim=0): in front of the weights' launch, which reads it
            zp8 = at::empty({rows, scale->size(1)}, packed->options().dtype(at::kChar));
            if (!packed->is_cpu() && g_unpack_dim0(static_cast<const int32_t*>(zpp->data_ptr()), zpp->size(0), zpp->size(1), rows, bits, static_cast<int8_t*>(zp8.data_ptr()),
                                                   reinterpret_cast<void*>(stream)) != 0)
                return false;
        }
        if (!packed->is_cpu() && g_unpack_dequant(static_cast<const int32_t*>(packed->data_ptr()), rows, packed->size(1), cols, bits, scale->data_ptr(), dt,
                                                  asym ? zp8.data_ptr() : nullptr, asym ? CT_I8 : -1, 1, group, cols / group,
                                                  cg.defined() ? static_cast<const int32_t*>(cg.data_ptr()) : nullptr, out.data_ptr(), dt, reinterpret_cast<void*>(stream)) != 0)
            return false;
        drop(e.params, N.weight_packed);
        if (asym) set_entry(e, N.weight_zero_point, zp8);  // unpacked, int8, in place
        set_entry(e, N.weight, out);
        set_status(m, status.ptr());
        return true;
    });
}

// mxfp8-quantized (reference compressors/mxfp8/base.py:29-118): float8 weights in groups of 32 — rows of the 8-bit tables, kind fp8 / fp8z — under 16-bit
// power-of-two scales that are STORED as E8M0 codes: a second table (the batch's aux rows; ct_mx_scale_batch) converts the scales, float -> code on the way
// in, code -> bfloat16 on the way back (launched BEFORE the weights' table, which reads the bfloat16 scales).  infos[i] (compress): 1 | drop mask << 1, or 0.
bool mx8_take_compress(PyObject* m, int64_t info, Entries& e, Sink& sink) {
    const int dropmask = (int)((info >> 1) & 7);
    if (!(info > 0 && (info & 1))) return false;
    const Q8Entries q(e);
    if (!q.ok) return false;
    const at::Tensor *w = q.w, *scale = q.scale, *zp = q.zp;
    const bool f8z = zp && zp->scalar_type() == at::kFloat8_e4m3fn;
    if (zp && !f8z) return false;
    const int64_t rows = w->size(0), cols = w->size(1);
    const int64_t group = q8_group(rows, cols, *scale, zp, w->scalar_type(), w->device(), 2, 32, f8z);
    if (group != 32 || !staying_entries_are_final(e, {N.weight, N.weight_scale}, dropmask)) return false;
    at::Tensor out = at::empty({rows, cols}, w->options().dtype(at::kFloat8_e4m3fn));
    at::Tensor codes = at::empty(scale->sizes(), scale->options().dtype(at::kByte));
    Batch& b = sink.at(*w, q8_code(w->scalar_type(), f8z ? 2 : 1, 8));
    b.row(item_row(w->data_ptr(), scale->data_ptr(), data_or_null(zp), out.data_ptr(), rows, cols, group));
    b.aux_row(item_row(scale->data_ptr(), nullptr, nullptr, codes.data_ptr(), scale->numel(), 1, 0));
    // (module, codes, scale codes, drop mask, keep-alive weight, keep-alive scale, keep-alive zero point or None)
    b.jobs.append(py::make_tuple(borrowed(m), wrap(out), wrap(codes), dropmask, entry_ref(e, N.weight), entry_ref(e, N.weight_scale),
                                 zp ? entry_ref(e, N.weight_zero_point) : py::none()));
    return true;
}

bool mx8_take_decompress(PyObject* m, int64_t, Entries& e, Sink& sink) {
    const at::Tensor *q = e.tensor(N.weight), *codes = e.tensor(N.weight_scale);
    if (!(q && codes && !e.has(N.weight_g_idx) && !e.has(N.weight_zero_point) && dense_source(*q) && q->scalar_type() == at::kFloat8_e4m3fn &&
          codes->scalar_type() == at::kByte && codes->device() == q->device() && codes->is_contiguous() && codes->dim() == 2))
        return false;
    const int64_t rows = q->size(0), cols = q->size(1);
    // (cols / 32 > 1: only this loop asks it — a single group per row is left to the Python path)
    if (!(rows > 0 && cols % 32 == 0 && codes->size(0) == rows && codes->size(1) == cols / 32 && cols / 32 > 1 && staying_entries_are_final(e, {N.weight, N.weight_scale})))
        return false;
    at::Tensor scale = at::empty(codes->sizes(), codes->options().dtype(at::kBFloat16));  // decompress_mx_scale: bfloat16, and so is the weight (mxfp8/base.py:74-101)
    at::Tensor out = at::empty({rows, cols}, scale.options());
    Batch& b = sink.at(*q, q8_code(at::kBFloat16, 1, 8));
    b.row(item_row(q->data_ptr(), scale.data_ptr(), nullptr, out.data_ptr(), rows, cols, 32));
    b.aux_row(item_row(codes->data_ptr(), nullptr, nullptr, scale.data_ptr(), codes->numel(), 1, 0));
    b.jobs.append(py::make_tuple(borrowed(m), wrap(out), wrap(scale), 0, entry_ref(e, N.weight), entry_ref(e, N.weight_scale), py::none()));
    return true;
}

// the scale is replaced where it is, `weight` is re-added last (mxfp8/base.py: the naive codec pops and re-adds it, the scale is assigned to its existing key)
void mx8_finish(py::list jobs, py::object status) {
    finish_jobs(jobs, status.ptr(), [](PyObject* job, Entries& e) {
        drop_zero_points(e, PyLong_AsLong(PyTuple_GET_ITEM(job, 3)));
        set_entry(e, N.weight_scale, job_tensor(job, 2));
        drop(e.params, N.weight);
        set_entry(e, N.weight, job_tensor(job, 1));
    });
}

// pack-quantized with num_bits = 8 and a symmetric weights-only scheme (the W8A16 preset; reference compressors/pack_quantized/base.py:62-163): the codes are
// the 8-bit tables' kind 3 (int8 + 128, four to an int32 word = pack_to_int32), the entries are the W4 ones (weight -> weight_packed + weight_shape), so the
// jobs have the W4 jobs' layout and go to w4_finish_compress / w4_finish_decompress.  infos[i]: group_size | strategy << 25 (0 tensor, 1 channel, 2 group), or < 0.
bool w8_take_compress(PyObject* m, int64_t info, Entries& e, Sink& sink) {
    if (info < 0 || dict_has(m, N.weight_packed) || dict_has(m, N.weight_shape)) return false;
    const Q8Entries q(e);
    // (a `weight_shape` left by an earlier decompress is overwritten in place, as in the W4 loop)
    if (!(q.ok && !e.has(N.weight_packed) && q.w->size(1) % 32 == 0)) return false;
    const at::Tensor *w = q.w, *zp = q.zp;
    const int64_t rows = w->size(0), cols = w->size(1);
    const int64_t group = q8_group(rows, cols, *q.scale, zp, w->scalar_type(), w->device(), (int)((info >> 25) & 3), info & 0xfffff, false);
    if (!(group > 0 && staying_entries_are_final(e, {N.weight, N.weight_zero_point}))) return false;
    at::Tensor packed = at::empty({rows, cols / 4}, w->options().dtype(at::kInt));
    Batch& b = sink.at(*w, q8_code(w->scalar_type(), 3, 8));
    b.row(item_row(w->data_ptr(), q.scale->data_ptr(), data_or_null(zp), packed.data_ptr(), rows, cols, group));
    // w4_finish_compress's job: (module, packed, rows, cols, keep-alive weight, zp_packed = None: the symmetric scheme's zero point is dropped, keep-alive zp)
    b.jobs.append(py::make_tuple(borrowed(m), wrap(packed), rows, cols, entry_ref(e, N.weight), py::none(), zp ? entry_ref(e, N.weight_zero_point) : py::none()));
    return true;
}

bool w8_take_decompress(PyObject* m, int64_t info, Entries& e, Sink& sink) {
    if (info < 0 || dict_has(m, N.weight)) return false;
    const at::Tensor *packed = e.tensor(N.weight_packed), *scale = e.tensor(N.weight_scale);
    int64_t rows = 0, cols = 0;
    if (!(packed && scale && !e.has(N.weight_g_idx) && !e.has(N.weight_zero_point) && !e.has(N.weight) && dense_source(*packed) && packed->scalar_type() == at::kInt &&
          stored_shape(e.tensor(N.weight_shape), rows, cols)))
        return false;
    if (!(cols % 32 == 0 && packed->size(0) == rows && packed->size(1) == cols / 4)) return false;
    // the layout is read off the scale's shape, as upstream's argument-free dequantize call does (pack_quantized/base.py:156-161, forward.py:99-130)
    const int64_t group = q8_group(rows, cols, *scale, nullptr, scale->scalar_type(), packed->device(), -1, 0, false);
    if (group == 0 || !staying_entries_are_final(e, {N.weight_packed})) return false;
    at::Tensor out = at::empty({rows, cols}, scale->options());
    Batch& b = sink.at(*packed, q8_code(scale->scalar_type(), 3, 8));
    b.row(item_row(packed->data_ptr(), scale->data_ptr(), nullptr, out.data_ptr(), rows, cols, group));
    // w4_finish_decompress's job: (module, out, keep-alive packed, zp = None, -)
    b.jobs.append(py::make_tuple(borrowed(m), wrap(out), entry_ref(e, N.weight_packed), py::none(), py::none()));
    return true;
}

// ------------------------------------------------------------------------------------------
// FP4 codecs (nvfp4-pack-quantized, group 16 under a global scale; mxfp4-pack-quantized, group 32; reference compressors/nvfp4/base.py:68-139,
// mxfp4/base.py:27-65): NVFP4PackedCompressor.compress_modules / decompress_modules in C++, as the W4 and 8-bit loops above — the table of
// `ct_fp4_quant_pack_batch` / `ct_fp4_unpack_dequant_batch` from the modules' own entries (struct ct_w4_item in its FP4 reading: zp = the module's global
// scale, zp_packed = the stored / bfloat16 scale output), one launch per window, then the dictionary delta of swap_direct_entries under the kernel: weight,
// weight_scale (and a symmetric scheme's zero points) leave, weight_packed and the stored weight_scale arrive — resp. the other way round.  The interpreter
// spent 14 us per module and direction on this with one launch per module (a TinyLlama-shaped NVFP4 tree ran at 0.13 of the HBM peak, an 8B-shaped one at 0.58).
// compress infos[i]: 1 | drop mask << 1 (weight / input / output zero point of a symmetric scheme) when the scheme stores its scale in the format's usual
// dtype; else 0.  batch key code: weights' dtype code | scales' dtype code << 4 (`dtype_code`); 0 on the way back (the outputs are bfloat16).
// ------------------------------------------------------------------------------------------
// the global scale as the kernel takes it: one float32 on the tensor's device (codec._gs_fast's no-op case)
inline bool plain_gs(const at::Tensor& g, const at::Device& dev) { return g.scalar_type() == at::kFloat && g.numel() == 1 && g.device() == dev && aligned(g, 4); }

// NVFP4 (group 16) has a global scale entry and it is the plain one; MXFP4 has none at all
inline bool fp4_global_scale_ok(const Entries& e, const at::Tensor* gs, int64_t group, const at::Device& dev) {
    return (gs != nullptr) == (group == 16) && tensor_or_absent(e, gs, g_weight_global_scale) && (!gs || plain_gs(*gs, dev));
}

bool fp4_take_compress(PyObject* m, int64_t info, Entries& e, Sink& sink, int64_t group) {
    const int dropmask = (int)((info >> 1) & 7);
    if (!(info > 0 && (info & 1)) || dict_has(m, N.weight_packed)) return false;
    const at::Tensor *w = e.tensor(N.weight), *scale = e.tensor(N.weight_scale), *gs = e.tensor(g_weight_global_scale);
    // (the kernel loads four 16-bit / two float32 scales at once: 8-byte aligned, not 16.  A zero point entry: dropped for a symmetric scheme; present under
    // an asymmetric one the Python path raises)
    if (!(w && scale && !e.has(N.weight_packed) && dense_source(*w) && half_type(w->scalar_type()) && fp4_global_scale_ok(e, gs, group, w->device()) &&
          scale->device() == w->device() && scale->is_contiguous() && aligned(*scale, 8) &&
          (half_type(scale->scalar_type()) || (group == 16 && scale->scalar_type() == at::kFloat)) && (e.tensor(N.weight_zero_point) == nullptr || (dropmask & 1))))
        return false;
    const int64_t rows = w->size(0), cols = w->size(1);
    if (!(rows > 0 && cols % group == 0 && (rows * cols) % 32 == 0 && scale->dim() == 2 && scale->size(0) == rows && scale->size(1) == cols / group &&
          staying_entries_are_final(e, {N.weight, N.weight_scale}, dropmask)))
        return false;
    at::Tensor packed = at::empty({rows, cols / 2}, w->options().dtype(at::kByte));
    at::Tensor stored = at::empty({rows, cols / group}, w->options().dtype(group == 16 ? at::kFloat8_e4m3fn : at::kByte));
    Batch& b = sink.at(*w, half_code(w->scalar_type()) | (dtype_code(scale->scalar_type()) << 4));
    b.row(item_row(w->data_ptr(), scale->data_ptr(), data_or_null(gs), packed.data_ptr(), rows, cols, group, stored.data_ptr()));
    // (module, packed bytes, stored scale, drop mask, keep-alive weight, keep-alive scale)
    b.jobs.append(py::make_tuple(borrowed(m), wrap(packed), wrap(stored), dropmask, entry_ref(e, N.weight), entry_ref(e, N.weight_scale)));
    return true;
}

bool fp4_take_decompress(PyObject* m, int64_t, Entries& e, Sink& sink, int64_t group) {
    if (dict_has(m, N.weight)) return false;
    const at::Tensor *packed = e.tensor(N.weight_packed), *scale = e.tensor(N.weight_scale), *gs = e.tensor(g_weight_global_scale);
    // (packed bytes: the kernel loads 4-byte words of them, not 16-byte units)
    if (!(packed && scale && !e.has(N.weight) && dense_source(*packed, 4) && packed->scalar_type() == at::kByte && fp4_global_scale_ok(e, gs, group, packed->device()) &&
          scale->device() == packed->device() && scale->is_contiguous() && scale->scalar_type() == (group == 16 ? at::kFloat8_e4m3fn : at::kByte)))
        return false;
    const int64_t rows = packed->size(0), cols = packed->size(1) * 2;
    if (!(rows > 0 && cols > 0 && cols % group == 0 && (rows * cols) % 32 == 0 && scale->dim() == 2 && scale->size(0) == rows && scale->size(1) == cols / group &&
          staying_entries_are_final(e, {N.weight_packed, N.weight_scale})))
        return false;
    at::Tensor out = at::empty({rows, cols}, packed->options().dtype(at::kBFloat16));  // unpack_fp4_from_uint8's default dtype (nvfp4/base.py:118-131)
    at::Tensor sout = at::empty({rows, cols / group}, packed->options().dtype(at::kBFloat16));
    Batch& b = sink.at(*packed, 0);
    b.row(item_row(packed->data_ptr(), scale->data_ptr(), data_or_null(gs), out.data_ptr(), rows, cols, group, sout.data_ptr()));
    b.jobs.append(py::make_tuple(borrowed(m), wrap(out), wrap(sout), 0, entry_ref(e, N.weight_packed), entry_ref(e, N.weight_scale)));
    return true;
}

// the entries arrive in the order swap_direct_entries leaves them: (weight_packed, weight_scale) resp. (weight_scale, weight)
void fp4_finish(py::list jobs, py::object status, bool compress) {
    finish_jobs(jobs, status.ptr(), [compress](PyObject* job, Entries& e) {
        const at::Tensor &a = job_tensor(job, 1), &sc = job_tensor(job, 2);  // a: packed bytes / dense weight
        drop(e.params, compress ? N.weight : N.weight_packed);
        drop(e.params, N.weight_scale);
        if (compress) {
            drop_zero_points(e, PyLong_AsLong(PyTuple_GET_ITEM(job, 3)));
            set_entry(e, N.weight_packed, a);
            set_entry(e, N.weight_scale, sc);
        } else {
            set_entry(e, N.weight_scale, sc);
            set_entry(e, N.weight, a);
        }
    });
}

// the Python-visible plan entries: names, arguments and return shapes as the compressors call them (compressors/*/base.py through run_planned)
py::tuple w4_plan_compress(py::list modules, py::object infos) { return plan_modules(modules, infos.ptr(), w4_take_compress); }
py::tuple w4_plan_decompress(py::list modules, py::object infos) { return plan_modules(modules, infos.ptr(), w4_take_decompress); }
py::tuple q8_plan_compress(py::list modules, py::object infos) { return plan_modules(modules, infos.ptr(), q8_take_compress); }
py::tuple q8_plan_decompress(py::list modules, py::object infos) { return plan_modules(modules, infos.ptr(), q8_take_decompress); }
py::tuple mx8_plan_compress(py::list modules, py::object infos) { return plan_modules(modules, infos.ptr(), mx8_take_compress); }
py::tuple mx8_plan_decompress(py::list modules) { return plan_modules(modules, nullptr, mx8_take_decompress); }
py::tuple w8_plan_compress(py::list modules, py::object infos) { return plan_modules(modules, infos.ptr(), w8_take_compress); }
py::tuple w8_plan_decompress(py::list modules, py::object infos) { return plan_modules(modules, infos.ptr(), w8_take_decompress); }
py::tuple fp4_plan_compress(py::list modules, py::object infos, int64_t group) {
    return plan_modules(modules, infos.ptr(), [group](PyObject* m, int64_t info, Entries& e, Sink& sink) { return fp4_take_compress(m, info, e, sink, group); });
}
py::tuple fp4_plan_decompress(py::list modules, int64_t group) {
    return plan_modules(modules, nullptr, [group](PyObject* m, int64_t info, Entries& e, Sink& sink) { return fp4_take_decompress(m, info, e, sink, group); });
}


// Marlin24Compressor.compress for an int4 scheme outside a deferred-check context, from the popped state-dict entries on: the layout tests
// of the one-launch path (compressors/sparse/marlin_24.py, same conditions), then marlin24_w4_full.  `group_size`: the scheme's, 0 for a
// channel-wise scheme, negative for a group scheme without a group size.  None when the tensors are not the one-launch case: the Python path takes the call.
py::object marlin24_compress_default(const at::Tensor& weight, const at::Tensor& scale, const c10::optional<at::Tensor>& zp, int64_t group_size, uintptr_t flag_host,
                                     uintptr_t flag_dev, uintptr_t verdict_ws, uintptr_t stream) {
    touch_tls();
    const bool channel = group_size == 0;
    if (group_size < 0 || !g_abi.marlin_full || !on_device(weight) || weight.dim() != 2 || !half_type(weight.scalar_type()) || !half_type(scale.scalar_type()) || scale.dim() < 1 ||
        scale.dim() > 2)
        return py::none();
    const int64_t m = weight.size(0), k = weight.size(1);
    if (m == 0 || m % 64 != 0 || k % 256 != 0 || k == 0 || !(channel || (group_size % 16 == 0 && k % group_size == 0)) || !weight.is_contiguous() || !aligned16(weight))
        return py::none();
    at::Tensor scale2d = scale.dim() == 2 ? scale : scale.reshape({scale.size(0), -1});
    if (!on_device(scale2d) || !scale2d.is_contiguous() || scale2d.device() != weight.device() || (m * scale2d.size(1)) % 64 != 0) return py::none();
    int zdt = -1;
    if (zp.has_value()) {
        zdt = dtype_code(zp->scalar_type());
        if (zdt < 0 || !on_device(*zp) || !zp->is_contiguous() || zp->device() != weight.device()) return py::none();
    }
    const int64_t group = (channel || group_size > k) ? k : group_size;
    const bool group_perm = !channel && group_size < k / 2;  // the in-dimension of the COMPRESSED weight decides (marlin_24.py: is_group)
    return marlin24_w4_full(weight, dtype_code(weight.scalar_type()), scale2d, dtype_code(scale2d.scalar_type()), zp, zdt, group, group_perm, flag_host, flag_dev, verdict_ws, stream);
}

}  // namespace

PYBIND11_MODULE(_hostpath, mod) {
    touch_tls();
    N.init();
    g_input_zero_point = PyUnicode_InternFromString("input_zero_point");
    g_output_zero_point = PyUnicode_InternFromString("output_zero_point");
    g_weight_global_scale = PyUnicode_InternFromString("weight_global_scale");
    py::module_ torch_mod = py::module_::import("torch");
    g_make_subclass = py::object(torch_mod.attr("Tensor").attr("_make_subclass")).release().ptr();
    g_parameter_cls = py::object(torch_mod.attr("nn").attr("Parameter")).release().ptr();
    g_module_setattr = py::object(torch_mod.attr("nn").attr("Module").attr("__setattr__")).release().ptr();
    g_module_delattr = py::object(torch_mod.attr("nn").attr("Module").attr("__delattr__")).release().ptr();
    mod.def("w4_plan_compress", &w4_plan_compress);
    mod.def("w4_finish_compress", &w4_finish_compress);
    mod.def("w4_plan_decompress", &w4_plan_decompress);
    mod.def("w4_finish_decompress", &w4_finish_decompress);
    mod.def("fp4_plan_compress", &fp4_plan_compress);
    mod.def("fp4_plan_decompress", &fp4_plan_decompress);
    mod.def("fp4_finish", &fp4_finish);
    mod.def("bind_pack", &bind_pack);
    mod.def("wb_compress_modules", &wb_compress_modules);
    mod.def("wb_decompress_modules", &wb_decompress_modules);
    mod.def("mx8_plan_compress", &mx8_plan_compress);
    mod.def("mx8_plan_decompress", &mx8_plan_decompress);
    mod.def("mx8_finish", &mx8_finish);
    mod.def("w8_plan_compress", &w8_plan_compress);
    mod.def("w8_plan_decompress", &w8_plan_decompress);
    mod.def("q8_plan_compress", &q8_plan_compress);
    mod.def("q8_plan_decompress", &q8_plan_decompress);
    mod.def("q8_finish", &q8_finish);
    mod.def("quantized_modules", &quantized_modules);
    mod.def("bind_abi", &bind_abi);
    mod.def("bitmask_compress", &bitmask_compress);
    mod.def("bitmask_compress_many", &bitmask_compress_many);
    mod.def("bitmask_decompress_many", &bitmask_decompress_many);
    mod.def("marlin24_w4_full", &marlin24_w4_full);
    mod.def("marlin24_compress_default", &marlin24_compress_default);
    mod.def("set_allow_cpu", [](bool v) { g_allow_cpu = v; });
    mod.def("set_wait_mode", [](int v) { g_wait_mode = v; });
    mod.attr("ITEM_WORDS") = kItemWords;
}

