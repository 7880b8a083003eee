//! rusty_sr -- Rust host over libsrhip (the MI355X engine).
//!
//!     rusty_sr <INPUT_FILE> <OUTPUT_FILE> [-p imagenet|imagenetlinear|anime|bilinear] [-c FILE] [-d] [--alpha [--bleed N]]
//!     rusty_sr validate [-p imagenet|imagenetlinear|anime | -c FILE] [-l] [-r] [-m N] [--metrics [--shave N]] <VALIDATION_FOLDER>
//!
//! Same arguments, progress text and failure text as millardjn/rusty_sr v1; decoding and encoding
//! of image files stay with the `image` crate as in the reference, everything between the decoded
//! pixels and the pixels to encode runs on the GPU.  `train` is not part of this host; its validation pass is (`validate`).
//! This file is not compiled in the repository's image (no Rust toolchain); the C++ twin
//! `rusty_sr_amd/host/main.cpp` is what the tests drive, and `tests/test_rust_host.py` keeps the
//! two in step (same option names, same strings, every FFI symbol exported).
extern crate image;

mod srhip;

use std::env;
use std::fs::File;
use std::io::{stdout, Read, Write};
use std::path::Path;
use std::process::exit;

use srhip::Engine;

static IMAGENET: &'static [u8] = include_bytes!("../../rusty_sr_amd/res/imagenet.rsr");
static IMAGENETLINEAR: &'static [u8] = include_bytes!("../../rusty_sr_amd/res/imagenetlinear.rsr");
static ANIME: &'static [u8] = include_bytes!("../../rusty_sr_amd/res/anime.rsr");

const BUILTIN: [&'static str; 4] = ["imagenet", "imagenetlinear", "anime", "bilinear"];

struct Options {
    input: String,
    output: String,
    parameters: Option<String>,
    custom: Option<String>,
    downsample: bool,
    device: i32,
    split_f16: bool,
    timing: bool,
    alpha: bool,
    bleed: i32,
}

fn usage_error(msg: &str) -> ! {
    let _ = writeln!(std::io::stderr(),
        "error: {}\n\nUSAGE:\n    rusty_sr [FLAGS] [OPTIONS] <INPUT_FILE> <OUTPUT_FILE>\n\nFor more information try --help", msg);
    exit(2)
}

fn die(msg: &str) -> ! {
    let _ = writeln!(std::io::stderr(), "error: {}", msg);
    exit(1)
}

fn parse_args() -> Options {
    let mut o = Options { input: String::new(), output: String::new(), parameters: None, custom: None,
                          downsample: false, device: 0, split_f16: false, timing: false, alpha: false,
                          bleed: srhip::SR_ALPHA_BLEED_DEFAULT };
    let mut has_bleed = false;
    let mut positional: Vec<String> = Vec::new();
    let mut args = env::args().skip(1);
    while let Some(a) = args.next() {
        let mut value = |name: &str| -> String {
            match args.next() {
                Some(v) => v,
                None => usage_error(&format!("The argument '{}' requires a value but none was supplied", name)),
            }
        };
        match a.as_str() {
            "train" if positional.is_empty() => {
                let _ = writeln!(std::io::stderr(), "error: the `train` sub-command is not part of this build");
                exit(2)
            }
            "-h" | "--help" => {
                println!("Rusty SR v0.1.1 (MI355X engine)\nUSAGE:\n    rusty_sr [-d] [-p PARAMETERS | -c PARAMETER_FILE] \
                          [--device N] [--precision f32|split_f16] [--timing] [--alpha [--bleed N]] <INPUT_FILE> <OUTPUT_FILE>\n\
                          \x20       --alpha         Keep transparency: bleed the visible colours under the transparent pixels, upscale, and\n\
                          \x20                       write the interpolated alpha channel (.png output only)\n\
                          \x20       --bleed <N>     with --alpha: how many pixels the colours are bled outward, 0..16 [default: 8]");
                exit(0)
            }
            "-V" | "--version" => {
                println!("Rusty SR v0.1.1");
                exit(0)
            }
            "-d" | "--downsample" => o.downsample = true,
            "--timing" => o.timing = true,
            "-p" | "--parameters" => o.parameters = Some(value("--parameters <PARAMETERS>")),
            "-c" | "--custom" => o.custom = Some(value("--custom <PARAMETER_FILE>")),
            "--device" => o.device = value("--device <N>").parse().unwrap_or_else(|_| usage_error("--device takes an integer")),
            "--precision" => {
                let v = value("--precision <MODE>");
                match v.as_str() {
                    "f32" => o.split_f16 = false,
                    "split_f16" => o.split_f16 = true,
                    _ => usage_error(&format!("'{}' isn't a valid value for '--precision <MODE>'", v)),
                }
            }
            "--alpha" => o.alpha = true,
            "--bleed" => {
                let v = value("--bleed <N>");
                match v.parse::<i32>() {
                    Ok(n) if n >= 0 && n <= srhip::SR_ALPHA_BLEED_MAX => o.bleed = n,
                    _ => usage_error(&format!("'{}' isn't a valid value for '--bleed <N>'\n\t[values: 0..16]", v)),
                }
                has_bleed = true;
            }
            "--metrics" | "--shave" => usage_error(&format!("The argument '{}' can only be used with the 'validate' subcommand", a)),
            // (`train` is not part of this host: its objective option, srhip::Engine::set_loss in the library, is refused by name)
            "--loss" => usage_error("The argument '--loss' can only be used with the 'train' subcommand"),
            "--lr" | "--lr-schedule" | "--warmup" | "--clip" | "--ema" | "--resume" => {
                usage_error(&format!("The argument '{}' can only be used with the 'train' subcommand", a))
            }
            s if s.len() > 1 && s.starts_with('-') => {
                usage_error(&format!("Found argument '{}' which wasn't expected, or isn't valid in this context", s))
            }
            _ => positional.push(a.clone()),
        }
    }
    if let Some(ref p) = o.parameters {
        if !BUILTIN.contains(&p.as_str()) {
            usage_error(&format!("'{}' isn't a valid value for '--parameters <PARAMETERS>'\n\t[values: anime, bilinear, imagenet, imagenetlinear]", p));
        }
    }
    if o.custom.is_some() && o.parameters.is_some() {
        usage_error("The argument '--custom <PARAMETER_FILE>' cannot be used with '--parameters <PARAMETERS>'");
    }
    if o.downsample && (o.custom.is_some() || o.parameters.is_some()) {
        usage_error("The argument '--downsample' cannot be used with '--parameters <PARAMETERS>' or '--custom <PARAMETER_FILE>'");
    }
    if positional.len() < 2 {
        usage_error("The following required arguments were not provided:\n    <INPUT_FILE>\n    <OUTPUT_FILE>");
    }
    if positional.len() > 2 {
        usage_error(&format!("Found argument '{}' which wasn't expected, or isn't valid in this context", positional[2]));
    }
    if has_bleed && !o.alpha {
        usage_error("The following required arguments were not provided:\n    --alpha");
    }
    if o.alpha && o.downsample {
        usage_error("The argument '--alpha' cannot be used with '--downsample'");
    }
    if o.alpha && !positional[1].to_lowercase().ends_with(".png") {
        usage_error("The argument '--alpha' cannot be used with an output file other than .png: JPEG, BMP and PPM carry no alpha channel");
    }
    o.input = positional[0].clone();
    o.output = positional[1].clone();
    o
}

fn validate_usage_error(msg: &str) -> ! {
    let _ = writeln!(std::io::stderr(),
        "error: {}\n\nUSAGE:\n    rusty_sr validate [FLAGS] [OPTIONS] <VALIDATION_FOLDER>\n\nFor more information try --help", msg);
    exit(2)
}

const DECODABLE: [&'static str; 13] = ["png", "jpg", "jpeg", "gif", "tif", "tiff", "bmp", "ico", "tga", "ppm", "pgm", "pbm", "pnm"];

fn collect_files(dir: &Path, recurse: bool, out: &mut Vec<std::path::PathBuf>) {
    let entries = match std::fs::read_dir(dir) {
        Ok(e) => e,
        Err(_) => die("could not read the validation folder"),
    };
    for entry in entries.filter_map(|e| e.ok()) {
        let path = entry.path();
        if path.is_dir() {
            if recurse {
                collect_files(&path, recurse, out);
            }
        } else if let Some(ext) = path.extension().and_then(|e| e.to_str()) {
            if DECODABLE.contains(&ext.to_lowercase().as_str()) {
                out.push(path);
            }
        }
    }
}

/// `rusty_sr validate`: the validation pass of the reference's `train` (main.rs:220-247) on its own, with `train`'s options
/// (main.rs:83-114).  Files are decoded on a second thread ahead of the GPU; PSNR = -10 log10(sum err / sum n) (main.rs:236-246).
fn validate(args: Vec<String>) {
    let (mut parameters, mut custom, mut folder): (Option<String>, Option<String>, Option<String>) = (None, None, None);
    let (mut linear, mut recurse, mut split_f16, mut timing, mut metrics) = (false, false, false, false, false);
    let mut val_max: Option<usize> = None;
    let mut shave: Option<i32> = None;  // --metrics: None = the factor
    let mut devices: Vec<i32> = Vec::new();
    let mut it = args.into_iter();
    while let Some(a) = it.next() {
        let mut value = |name: &str| -> String {
            match it.next() {
                Some(v) => v,
                None => validate_usage_error(&format!("The argument '{}' requires a value but none was supplied", name)),
            }
        };
        match a.as_str() {
            "-h" | "--help" => {
                println!("USAGE:\n    rusty_sr validate [-l|--linearLoss] [-r|--recurse] [-m|--val_max N] [-p PARAMETERS | -c PARAMETER_FILE] \
                          [--precision f32|split_f16] [--devices N,N,...] [--timing] [--metrics [--shave N]] <VALIDATION_FOLDER>");
                exit(0)
            }
            "-l" | "--linearLoss" => linear = true,
            "-r" | "--recurse" => recurse = true,
            "--timing" => timing = true,
            "--metrics" => metrics = true,
            "--shave" => {
                let v = value("--shave <N>");
                match v.parse::<i32>() {
                    Ok(n) if n >= 0 => shave = Some(n),
                    _ => validate_usage_error(&format!("'{}' isn't a valid value for '--shave <N>'", v)),
                }
            }
            "-d" | "--downsample" => validate_usage_error("The argument '--downsample' cannot be used with 'validate'"),
            "--loss" => validate_usage_error("The argument '--loss' can only be used with the 'train' subcommand"),
            "--lr" | "--lr-schedule" | "--warmup" | "--clip" | "--ema" | "--resume" => {
                validate_usage_error(&format!("The argument '{}' can only be used with the 'train' subcommand", a))
            }
            "-p" | "--parameters" => parameters = Some(value("--parameters <PARAMETERS>")),
            "-c" | "--custom" => custom = Some(value("--custom <PARAMETER_FILE>")),
            "-m" | "--val_max" => {
                let v = value("--val_max <N>");
                match v.parse::<usize>() {
                    Ok(n) if n > 0 => val_max = Some(n),
                    _ => validate_usage_error("-val_max N must be a positive integer"),
                }
            }
            "--devices" => {
                let v = value("--devices <N,N,...>");
                for d in v.split(',') {
                    devices.push(d.parse().unwrap_or_else(|_| validate_usage_error(&format!("'{}' isn't a valid value for '--devices <N,N,...>'", v))));
                }
            }
            "--precision" => {
                let v = value("--precision <MODE>");
                match v.as_str() {
                    "f32" => split_f16 = false,
                    "split_f16" => split_f16 = true,
                    _ => validate_usage_error(&format!("'{}' isn't a valid value for '--precision <MODE>'", v)),
                }
            }
            s if s.len() > 1 && s.starts_with('-') => {
                validate_usage_error(&format!("Found argument '{}' which wasn't expected, or isn't valid in this context", s))
            }
            _ if folder.is_none() => folder = Some(a.clone()),
            _ => validate_usage_error(&format!("Found argument '{}' which wasn't expected, or isn't valid in this context", a)),
        }
    }
    if let Some(ref p) = parameters {
        if p != "imagenet" && p != "imagenetlinear" && p != "anime" {
            validate_usage_error(&format!("'{}' isn't a valid value for '--parameters <PARAMETERS>'\n\t[values: anime, imagenet, imagenetlinear]", p));
        }
    }
    if custom.is_some() && parameters.is_some() {
        validate_usage_error("The argument '--custom <PARAMETER_FILE>' cannot be used with '--parameters <PARAMETERS>'");
    }
    let folder = folder.unwrap_or_else(|| validate_usage_error("The following required arguments were not provided:\n    <VALIDATION_FOLDER>"));
    if shave.is_some() && !metrics {
        validate_usage_error("The following required arguments were not provided:\n    --metrics");
    }
    if !Path::new(&folder).is_dir() {
        validate_usage_error(&format!("'{}' is not a folder", folder));
    }
    let mut files = Vec::new();
    collect_files(Path::new(&folder), recurse, &mut files);
    files.sort_by(|a, b| a.as_os_str().to_string_lossy().as_bytes().cmp(b.as_os_str().to_string_lossy().as_bytes()));
    if let Some(n) = val_max {
        files.truncate(n);
    }
    if files.is_empty() {
        validate_usage_error(&format!("no image files in '{}'", folder));
    }
    if devices.is_empty() {
        devices.push(0);
    }

    let (params, banner): (Vec<f32>, &str) = if let Some(ref file) = custom {
        let mut data = Vec::new();
        File::open(Path::new(file)).and_then(|mut f| f.read_to_end(&mut data)).unwrap_or_else(|_| die("Error opening parameter file"));
        (decode_or_die(&data), "Validating using custom neural net parameters...")
    } else {
        match parameters.as_ref().map(|s| s.as_str()).unwrap_or("imagenet") {
            "imagenetlinear" => (decode_or_die(IMAGENETLINEAR), "Validating using linear loss imagenet neural net parameters..."),
            "anime" => (decode_or_die(ANIME), "Validating using anime neural net parameters..."),
            _ => (decode_or_die(IMAGENET), "Validating using imagenet neural net parameters..."),
        }
    };
    println!("{} {} image{}{}", banner, files.len(), if files.len() == 1 { "" } else { "s" }, if linear { ", linear loss" } else { "" });
    let factor = [3, 2, 4].iter().cloned().find(|&f| unsafe { srhip::sr_num_params_factor(f) } as usize == params.len()).unwrap_or(3);
    let mut engines: Vec<Engine> = devices.iter().map(|&d| Engine::new_factor(&params, factor, d).unwrap_or_else(|e| die(&e))).collect();
    for e in engines.iter_mut() {
        if split_f16 {
            e.set_precision(srhip::SR_PRECISION_SPLIT_F16).unwrap_or_else(|err| die(&err));
        }
    }

    // decode ahead of the GPU on a second thread, in path order
    let (tx, rx) = std::sync::mpsc::sync_channel(4);
    let names = files.clone();
    let decoder = std::thread::spawn(move || {
        for f in names {
            let img = image::open(&f).map(|i| i.to_rgba());
            if tx.send((f, img)).is_err() {
                return;
            }
        }
    });
    let t0 = std::time::Instant::now();
    let (mut err_sum, mut n_sum) = (0f64, 0f64);
    let (mut y_sum, mut y_n, mut s_sum, mut s_n) = (0f64, 0usize, 0f64, 0usize);  // --metrics: per-image means
    for (i, (path, img)) in rx.iter().enumerate() {
        let rgba = img.unwrap_or_else(|_| die(&format!("Error opening validation image file {}", path.display())));
        let (w, h) = rgba.dimensions();
        let k = i % engines.len();
        let (e, n) = if metrics {
            let (e, n, m) = engines[k].validation_metrics(&rgba.into_raw(), w, h, linear, 0, shave.unwrap_or(-1))
                .unwrap_or_else(|err| die(&format!("{}: {}", path.display(), err)));
            if m.y_count > 0 {
                y_sum += if m.y_sq_err == 0 { std::f64::INFINITY } else { 10.0 * (65025.0 * m.y_count as f64 / m.y_sq_err as f64).log10() };
                y_n += 1;
            } else {
                let _ = writeln!(std::io::stderr(), "{}: nothing left after the shave, left out of Y-PSNR", path.display());
            }
            if m.ssim_count > 0 {
                s_sum += m.ssim_sum / m.ssim_count as f64;
                s_n += 1;
            } else {
                let _ = writeln!(std::io::stderr(), "{}: too small for an 11x11 window after the shave, left out of SSIM", path.display());
            }
            (e, n)
        } else {
            engines[k].validation_error(&rgba.into_raw(), w, h, linear).unwrap_or_else(|err| die(&format!("{}: {}", path.display(), err)))
        };
        err_sum += e;
        n_sum += n as f64;
    }
    let _ = decoder.join();
    let psnr = if err_sum == 0.0 { std::f32::INFINITY } else { (-10.0 * (err_sum / n_sum).log10()) as f32 };
    println!("Validation PSNR:\t{}", psnr);  // main.rs:246
    if metrics {
        println!("Y-PSNR:\t{}", if y_n > 0 { (y_sum / y_n as f64) as f32 } else { std::f32::NAN });
        println!("SSIM:\t{}", if s_n > 0 { (s_sum / s_n as f64) as f32 } else { std::f32::NAN });
    }
    if timing {
        let s = t0.elapsed().as_secs_f64();
        let _ = writeln!(std::io::stderr(), "[timing] {} images in {:.3} s: {:.2} images/s", files.len(), s, files.len() as f64 / s);
    }
}

fn decode_or_die(blob: &[u8]) -> Vec<f32> {
    srhip::rsr_decode(blob).unwrap_or_else(|_| die("ByteVec conversion failed"))
}

fn main() {
    let argv: Vec<String> = env::args().collect();
    if argv.len() >= 2 && argv[1] == "validate" {
        validate(argv[2..].to_vec());
        return;
    }
    let o = parse_args();

    // which graph, which parameters -- and the line the reference prints for each choice
    let (graph, params, banner): (i32, Vec<f32>, &str) = if let Some(ref file) = o.custom {
        let mut data = Vec::new();
        File::open(Path::new(file)).and_then(|mut f| f.read_to_end(&mut data)).unwrap_or_else(|_| die("Error opening parameter file"));
        (srhip::SR_GRAPH_SR_NET, decode_or_die(&data), "Upscaling using custom neural net parameters...")
    } else if o.downsample {
        (srhip::SR_GRAPH_DOWNSAMPLE, Vec::new(), "Downsampling using average pooling of linear RGB values...")
    } else {
        match o.parameters.as_ref().map(|s| s.as_str()).unwrap_or("imagenet") {
            "imagenetlinear" => (srhip::SR_GRAPH_SR_NET, decode_or_die(IMAGENETLINEAR), "Upscaling using linear loss imagenet neural net parameters..."),
            "anime" => (srhip::SR_GRAPH_SR_NET, decode_or_die(ANIME), "Upscaling using anime neural net parameters..."),
            "bilinear" => (srhip::SR_GRAPH_BILINEAR, Vec::new(), "Upscaling using bilinear interpolation..."),
            _ => (srhip::SR_GRAPH_SR_NET, decode_or_die(IMAGENET), "Upscaling using imagenet neural net parameters..."),
        }
    };
    print!("{}", banner);
    let _ = stdout().flush();

    // a wrong parameter count comes back as SR_E_PARAM_COUNT, whose text is the reference's assert message
    let mut engine = Engine::new(graph, &params, o.device).unwrap_or_else(|e| die(&e));
    if graph == srhip::SR_GRAPH_SR_NET && o.split_f16 {
        engine.set_precision(srhip::SR_PRECISION_SPLIT_F16).unwrap_or_else(|e| die(&e));
    }

    let rgba = image::open(Path::new(&o.input)).unwrap_or_else(|_| die("Error opening input image file.")).to_rgba();
    let (w, h) = rgba.dimensions();
    let out = if o.alpha {
        engine.upscale_rgba8_alpha(&rgba.into_raw(), w, h, o.bleed).unwrap_or_else(|e| die(&e))
    } else {
        engine.upscale_rgba8(&rgba.into_raw(), w, h).unwrap_or_else(|e| die(&e))
    };
    if o.timing {
        let (total, h2d, d2h) = engine.last_timing();
        let _ = writeln!(std::io::stderr(), "\n[timing] kernels {:.3} ms, h2d {:.3} ms, d2h {:.3} ms", total, h2d, d2h);
    }

    print!(" Writing file...");
    let _ = stdout().flush();
    let (ow, oh) = engine.out_dims(w, h);
    let img = image::RgbaImage::from_raw(ow, oh, out).expect("engine returned a full RGBA8 buffer");
    img.save(Path::new(&o.output)).unwrap_or_else(|_| die("Could not write output file"));
    println!(" Done");
}
